#pragma once
// Kernels of the solo sparse solver: the row functors, the plain CSR-stream SpMV with its row-reduction companions,
// the value scaling of the equilibration and the exact-residual helper.  (The tiled lane-stream SpMV: sell.h.)
//
// Included by sparse.hip only -- the anonymous namespace keeps every kernel in that translation unit.
#include "reduce.h"
#include "sell.h"

namespace pogs_amd {
namespace {

constexpr int kSpTpb = 256;
constexpr int kSpCap = 4096;       // non-zeros staged in LDS per row block
constexpr int kSpMaxRows = 2048;   // rows per block cap (balance when rows are empty)

// ---------------------------------------------------------------------------
// Row functors (one thread per finished row; scalars accumulate in doubles)
// ---------------------------------------------------------------------------
template <typename T>
struct SpAxpbyOp {  // y[i] = alpha * dot + beta * yin[i]
  static constexpr int NS = 0;
  T alpha, beta;
  const T *yin;
  T *y;
  template <int N>
  __device__ __forceinline__ void row(int i, T dot, double (&)[N]) const {
    T v = alpha * dot;
    if (beta != static_cast<T>(0)) v += beta * yin[i];
    y[i] = v;
  }
};

template <typename T>
struct SpStoreOp {  // y[i] = dot, no sums: the local part of a row-sharded A^T product, before its all-reduce
  static constexpr int NS = 0;
  T *y;
  template <int N>
  __device__ __forceinline__ void row(int i, T dot, double (&)[N]) const { y[i] = dot; }
  struct In {};
  __device__ __forceinline__ In load(int) const { return In{}; }
  template <int N>
  __device__ __forceinline__ void apply(int i, T dot, const In &, double (&)[N]) const { y[i] = dot; }
};

template <typename T>
struct SpAxpbyNormOp {  // y[i] = alpha * dot + beta * yin[i]; s0 += y[i]^2
  static constexpr int NS = 1;
  T alpha, beta;
  const T *yin;
  T *y;
  template <int N>
  __device__ __forceinline__ void row(int i, T dot, double (&s)[N]) const {
    T v = alpha * dot;
    if (beta != static_cast<T>(0)) v += beta * yin[i];
    y[i] = v;
    dev::prod_acc(s[0], v, v);
  }
  // the same in two steps (sell.h: spmv_sell_fin_kernel requests the operands of several rows
  // before it uses any)
  struct In { T yin; };
  __device__ __forceinline__ In load(int i) const { return In{beta != static_cast<T>(0) ? yin[i] : static_cast<T>(0)}; }
  template <int N>
  __device__ __forceinline__ void apply(int i, T dot, const In &in, double (&s)[N]) const {
    T v = alpha * dot;
    if (beta != static_cast<T>(0)) v += beta * in.yin;
    y[i] = v;
    dev::prod_acc(s[0], v, v);
  }
};

template <typename T>
struct SpSkOp {  // out[i] = num / (dot + c)   (equil_helper.h:149-162)
  static constexpr int NS = 1;
  T num, c;
  T *out;
  // common-factor probe, see SkColOp in ops.h: sums new / old, stamps *mark when an entry's ratio
  // leaves r_ref by more than tol
  double *mark = nullptr;
  double stamp = 0;
  T tol = 0;
  T r_ref = 0;
  template <int N>
  __device__ __forceinline__ void row(int i, T dot, double (&s)[N]) const {
    const T v = num / (dot + c);
    const T old = out[i];
    const T r = old > static_cast<T>(0) ? v / old : static_cast<T>(0);
    s[0] += static_cast<double>(r);
    if (mark && !(fabs(r - r_ref) <= tol * r_ref)) *mark = stamp;
    out[i] = v;
  }
};

template <typename T>
struct SpTailOp {  // ProjTailOp for the y half: see ops.h
  static constexpr int NS = 2;
  T *znew;
  const T *zprev, *z12;
  T *ztemp;
  template <int N>
  __device__ __forceinline__ void row(int i, T dot, double (&s)[N]) const {
    znew[i] = dot;
    const T a = zprev[i] - dot, b = z12[i] - dot;
    dev::prod_acc(s[0], a, a);
    dev::prod_acc(s[1], b, b);
    ztemp[i] -= dot;
  }
  struct In { T zprev, z12, ztemp; };
  __device__ __forceinline__ In load(int i) const { return In{zprev[i], z12[i], ztemp[i]}; }
  template <int N>
  __device__ __forceinline__ void apply(int i, T dot, const In &in, double (&s)[N]) const {
    znew[i] = dot;
    const T a = in.zprev - dot, b = in.z12 - dot;
    dev::prod_acc(s[0], a, a);
    dev::prod_acc(s[1], b, b);
    ztemp[i] = in.ztemp - dot;
  }
};

template <typename T>
struct SpExactROp {  // r_i = (A x12)_i - y12_i (pogs.cpp:353-364)
  static constexpr int NS = 1;
  const T *y12;
  template <int N>
  __device__ __forceinline__ void row(int i, T dot, double (&s)[N]) const {
    const T r = dot - y12[i];
    dev::prod_acc(s[0], r, r);
  }
};

template <typename T>
struct SpExactSOp {  // s_j = (A^T u)_j + x12_j + c xt_j - xprev_j (pogs.cpp:366-373)
  static constexpr int NS = 1;
  const T *x12, *xt, *xprev;
  T zt_scale;
  template <int N>
  __device__ __forceinline__ void row(int j, T dot, double (&s)[N]) const {
    const T v = dot + x12[j] + zt_scale * xt[j] - xprev[j];
    dev::prod_acc(s[0], v, v);
  }
};

// ---------------------------------------------------------------------------
// SpMV kernel (CSR-stream with LDS staging)
// ---------------------------------------------------------------------------
template <typename T>
struct Csr {
  const T *val;
  const int *ind, *ptr, *blocks;
  int nrows, nblocks;
};

template <typename T, bool SQ, typename Op>
__global__ void __launch_bounds__(kSpTpb) spmv_kernel(Csr<T> A, const T *__restrict__ x, const double *x_nrm2,
                                                      Op op, double *scalar_partials) {
  constexpr int NS = Op::NS > 0 ? Op::NS : 1;
  __shared__ T s_prod[kSpCap];
  __shared__ T s_long[kSpTpb / 64];
  __shared__ double s_red[NS * (kSpTpb / 64)];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  double sacc[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) sacc[k] = 0.0;
  T xs = 1;
  if (x_nrm2) xs = static_cast<T>(1.0 / sqrt(*x_nrm2));

  for (int b = blockIdx.x; b < A.nblocks; b += gridDim.x) {
    const int r0 = A.blocks[b], r1 = A.blocks[b + 1];
    const int p0 = A.ptr[r0], p1 = A.ptr[r1];
    const int cnt = p1 - p0;
    if (cnt > kSpCap) {
      // one long row: the whole workgroup strides over it
      T s = 0;
      for (int k = t; k < cnt; k += kSpTpb) {
        T v = A.val[p0 + k];
        if (SQ) v *= v;
        s = sell_fma(v, x[A.ind[p0 + k]] * xs, s);
      }
      s = dev::wave_sum(s);
      if (lane == 0) s_long[wave] = s;
      __syncthreads();
      if (t == 0) {
        T tot = 0;
#pragma unroll
        for (int w = 0; w < kSpTpb / 64; ++w) tot += s_long[w];
        op.row(r0, tot, sacc);
      }
      __syncthreads();
      continue;
    }
    // stage val * x[ind] in LDS: 8 independent coalesced value/index loads and 8
    // gathers in flight per thread
    constexpr int U = 8;
    for (int k0 = 0; k0 < cnt; k0 += kSpTpb * U) {
      T v[U];
      int id[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int k = k0 + u * kSpTpb + t;
        const bool ok = k < cnt;
        v[u] = ok ? A.val[p0 + k] : static_cast<T>(0);
        id[u] = ok ? A.ind[p0 + k] : 0;
      }
      T xg[U];
#pragma unroll
      for (int u = 0; u < U; ++u) xg[u] = x[id[u]];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int k = k0 + u * kSpTpb + t;
        if (k < cnt) s_prod[k] = (SQ ? v[u] * v[u] : v[u]) * (xg[u] * xs);
      }
    }
    __syncthreads();
    const int nrows = r1 - r0;
    int tpr = 1;  // threads per row: a power of two <= 64, about a quarter of the mean row length
    while (tpr < 64 && tpr * 4 < cnt / (nrows > 0 ? nrows : 1)) tpr <<= 1;
    const int rpp = kSpTpb / tpr, lir = t % tpr, slot = t / tpr;
    for (int base = 0; base < nrows; base += rpp) {
      const int r = r0 + base + slot;
      T s = 0;
      if (r < r1) {
        const int a = A.ptr[r] - p0, e = A.ptr[r + 1] - p0;
        for (int k = a + lir; k < e; k += tpr) s += s_prod[k];
      }
      for (int off = tpr >> 1; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
      if (lir == 0 && r < r1) op.row(r, s, sacc);
    }
    __syncthreads();
  }
  if (Op::NS > 0) {
    dev::block_sum<NS, kSpTpb>(sacc, s_red);
    if (t == 0) {
#pragma unroll
      for (int k = 0; k < NS; ++k) scalar_partials[static_cast<size_t>(blockIdx.x) * NS + k] = sacc[k];
    }
  }
}

// row r: sum of its ncb partial sums (one per column group) in group order, then the row functor
// (Measured and not kept: letting the workgroup that finishes last -- a device counter -- add the
// scalar partials and form the CGLS scalar, in place of the launch_sum_cg launch that follows.
// 2048 workgroups incrementing one address serialise in L2: +50 us per SpMV.)
template <typename T, typename Op>
__global__ void __launch_bounds__(256) reduce_parts_kernel(const T *__restrict__ part, int nrows, int ncb, Op op,
                                                           double *scalar_partials) {
  constexpr int NS = Op::NS > 0 ? Op::NS : 1;
  __shared__ double s_red[NS * 4];
  double sacc[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) sacc[k] = 0.0;
  for (int r = blockIdx.x * 256 + threadIdx.x; r < nrows; r += gridDim.x * 256) {
    T sum = part[r];
    for (int cb = 1; cb < ncb; ++cb) sum += part[static_cast<size_t>(cb) * nrows + r];
    op.row(r, sum, sacc);
  }
  if (Op::NS > 0) {
    dev::block_sum<NS, 256>(sacc, s_red);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int k = 0; k < NS; ++k) scalar_partials[static_cast<size_t>(blockIdx.x) * NS + k] = sacc[k];
    }
  }
}

// the row functor applied to a finished vector of dot products (row-sharded solves: the
// A^T products are summed over the ranks before the functor sees them)
template <typename T, typename Op>
__global__ void __launch_bounds__(256) apply_rows_kernel(const T *__restrict__ dots, int nrows, Op op,
                                                         double *scalar_partials) {
  constexpr int NS = Op::NS > 0 ? Op::NS : 1;
  __shared__ double s_red[NS * 4];
  double sacc[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) sacc[k] = 0.0;
  for (int r = blockIdx.x * 256 + threadIdx.x; r < nrows; r += gridDim.x * 256) op.row(r, dots[r], sacc);
  if (Op::NS > 0) {
    dev::block_sum<NS, 256>(sacc, s_red);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int k = 0; k < NS; ++k) scalar_partials[static_cast<size_t>(blockIdx.x) * NS + k] = sacc[k];
    }
  }
}

// val[k] *= drow[row] * ecol[ind[k]], one wavefront per row; partial sum of squares
template <typename T>
__global__ void __launch_bounds__(256) scale_csr_kernel(T *val, const int *ind, const int *ptr, int nrows,
                                                        const T *drow, const T *ecol, double *partials) {
  __shared__ double s_red[4];
  const int lane = threadIdx.x & 63;
  const int w = (blockIdx.x * 256 + threadIdx.x) >> 6, nw = (gridDim.x * 256) >> 6;
  double acc[1] = {0.0};
  for (int r = w; r < nrows; r += nw) {
    const T dr = drow[r];
    for (int k = ptr[r] + lane; k < ptr[r + 1]; k += 64) {
      const T v = val[k] * (dr * ecol[ind[k]]);
      val[k] = v;
      dev::prod_acc(acc[0], v, v);
    }
  }
  dev::block_sum<1, 256>(acc, s_red);
  if (threadIdx.x == 0) partials[blockIdx.x] = acc[0];
}

// u = y12 + c yt - yprev   (pogs.cpp:366-368, y half)
template <typename T>
__global__ void exact_u_kernel(int m, const T *y12, const T *yt, const T *yprev, T c, T *u) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < m) u[i] = y12[i] + c * yt[i] - yprev[i];
}

}  // namespace
}  // namespace pogs_amd

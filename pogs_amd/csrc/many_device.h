// The device half of the many-problem solves (many_kernels.hip includes it): the structs the kernels
// take, many_problem(), the workgroup building blocks and the eight kernels.  The anonymous namespace keeps them local
// to that one translation unit.  Shapes, the workspace layout and the ragged table's rows are many_plan.h's.
#pragma once
#include "engine.h"
#include "many_plan.h"
#include "prox.h"
#include "reduce.h"

namespace pogs_amd {
namespace {

constexpr int kTPB = 256;
constexpr int kWaves = kTPB / 64;

// One function vector on the device: a field is an array or one value for every element (PogsAmdFn's broadcast).
template <typename T>
struct ManyFn {
  const T *p[5];   // a, b, c, d, e
  const int *h;
  T v[5];
  int h0;
  __device__ __forceinline__ T get(int f, int i) const { return p[f] ? p[f][i] : v[f]; }
  __device__ __forceinline__ int code(int i) const { return h ? h[i] : h0; }
};

// Per-problem setup scalars.
template <typename T>
struct ManyState {
  T nrmA, ne_est;
  int ne_iter, ne_done, stopped, pad;
};

// A kernel's arguments: the shape and workspace layout (many_offsets fills the base: the call's shape or, ragged, each
// problem's own) and the pools.
template <typename T>
struct ManyArgs : ManyLayout {
  T *ws;
  const T *src;                  // the chunk's input matrices, problem q at q*m*n (ragged: at prob[q].src)
  int rowmaj;
  const T *rnd;                  // Norm2Est start vector (n)
  const ManyFn<T> *fn;           // f of problem q at 2q, g at 2q + 1
  AdmmControl<T> *ctl;
  ManyState<T> *st;
  unsigned *done_count;
  T ce, cd;                      // Sinkhorn-Knopp regularisers (equil_helper.h:152-160)
  T *xo, *yo, *lo, *muo;         // chunk outputs, problem q at q*n / q*m (ragged: at prob[q].xo / .yo)
  double *optval;
  unsigned *iters;
  int *status;
  const ManyProb<T> *prob;       // ragged: one row per problem; nullptr: every problem m x n, problem q at q * stride
  size_t src0;                   // ragged: the element offset (as the rows' src counts) of the matrix src points at
};

// Problem q's view of the arguments, taken once at the top of every kernel: afterwards a.m, a.n, a.k, a.tall and the
// offsets are the problem's own, and ws, src, xo, yo, lo, muo point at the problem's own data (the per-problem arrays
// fn, ctl, st, optval, iters and status stay indexed by q).  Uniform (prob == nullptr): the shape is the kernel-wide
// one and the pointers advance by q problems.  Returns the problem's bound on the iterations of one loop launch.
// Everything here is uniform over the workgroup.
template <typename T>
__device__ __forceinline__ int many_problem(ManyArgs<T> &a, int q) {
  if (!a.prob) {
    a.ws += q * a.stride;
    a.src += q * (static_cast<size_t>(a.m) * a.n);
    a.xo += static_cast<size_t>(q) * a.n; a.muo += static_cast<size_t>(q) * a.n;
    a.yo += static_cast<size_t>(q) * a.m; a.lo += static_cast<size_t>(q) * a.m;
    return kMaxIterPerLaunch;
  }
  const ManyProb<T> p = a.prob[q];
  many_offsets(a, p.m, p.n);
  a.ce = p.ce; a.cd = p.cd;
  a.ws += p.ws;
  a.src += p.src - a.src0;
  a.xo += p.xo; a.muo += p.xo;
  a.yo += p.yo; a.lo += p.yo;
  return p.ipl;
}

// ---- workgroup building blocks -------------------------------------------------------------------

// NS double sums over the workgroup, the totals in every thread.  red: NS * (kWaves + 1) doubles.
template <int NS>
__device__ __forceinline__ void wg_sum(double (&v)[NS], double *red) {
  dev::block_sum<NS, kTPB>(v, red);
  if (threadIdx.x == 0)
    for (int q = 0; q < NS; ++q) red[NS * kWaves + q] = v[q];
  __syncthreads();
  for (int q = 0; q < NS; ++q) v[q] = red[NS * kWaves + q];
  __syncthreads();
}

// out(i, s), s = sum_{c < len(i)} M[i ld + c] v[c] (SQ: M^2 v) for the rows i < rows: one wavefront per row, lanes over
// the columns, the lanes' partials summed by the butterfly.  Call from all threads; no barrier inside.
template <typename T, bool SQ, typename Len, typename Out>
__device__ __forceinline__ void row_dots(const T *M, size_t ld, int rows, Len len, const T *v, Out out) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int i = w; i < rows; i += kWaves) {
    const T *r = M + static_cast<size_t>(i) * ld;
    const int L = len(i);
    T acc = 0;
    for (int c = lane; c < L; c += 64) {
      const T a = r[c];
      acc += SQ ? (a * a) * v[c] : a * v[c];
    }
    acc = dev::wave_sum(acc);
    if (lane == 0) out(i, acc);
  }
}

// out(c, s), s = sum_{r0(c) <= i < rows} M[i ld + c] v[i] (SQ: M^2 v) for the columns c < cols: a thread per column,
// and for narrow matrices (cols <= 128) 2 or 4 thread groups over interleaved rows whose partials are added in group
// order.  Call from all threads; ends with the outputs written (not yet visible: the caller syncs).  part: kTPB T.
template <typename T, bool SQ, typename R0, typename Out>
__device__ __forceinline__ void col_dots(const T *M, size_t ld, int rows, int cols, R0 r0, const T *v, Out out,
                                         T *part) {
  const int CP = cols >= kTPB ? kTPB : (cols + 63) / 64 * 64;
  const int RG = kTPB / CP;
  const int t = threadIdx.x, cc = t % CP, rg = t / CP;
  for (int c0 = 0; c0 < cols; c0 += CP) {
    const int c = c0 + cc;
    T acc = 0;
    if (rg < RG && c < cols) {
      for (int i = r0(c) + rg; i < rows; i += RG) {
        const T a = M[static_cast<size_t>(i) * ld + c];
        acc += SQ ? (a * a) * v[i] : a * v[i];
      }
    }
    if (RG > 1) {
      part[t] = acc;
      __syncthreads();
      if (rg == 0 && c < cols) {
        T s = part[cc];
        for (int q = 1; q < RG; ++q) s += part[q * CP + cc];
        out(c, s);
      }
      __syncthreads();
    } else if (rg == 0 && c < cols) {
      out(c, acc);
    }
  }
}

// The scaled function of element i (PogsObjectiveSeparable::scale, pogs.cpp:608-617, after FunctionObj's clamp of
// c and e, prox_lib.h:62-69): f by 1 / d_i (isf), g by e_j.
template <typename T>
struct Coef {
  T a, b, c, d, e;
  int h;
};
template <typename T>
__device__ __forceinline__ Coef<T> coef(const ManyFn<T> &F, int i, T s, bool isf) {
  Coef<T> r;
  r.h = F.code(i);
  r.a = F.get(0, i); r.b = F.get(1, i); r.c = F.get(2, i); r.d = F.get(3, i); r.e = F.get(4, i);
  r.c = r.c < static_cast<T>(0) ? static_cast<T>(0) : r.c;
  r.e = r.e < static_cast<T>(0) ? static_cast<T>(0) : r.e;
  if (isf) {
    r.a = r.a / s; r.d = r.d / s; r.e = r.e / (s * s);
  } else {
    r.a = r.a * s; r.d = r.d * s; r.e = r.e * (s * s);
  }
  return r;
}

// ---- setup ------------------------------------------------------------------------------------------

// A_j (row- or column-major input) into the problem's row-major copy.  grid (blocks, problems)
template <typename T>
__global__ __launch_bounds__(kTPB) void many_copy_kernel(ManyArgs<T> a) {
  const int q = blockIdx.y;
  many_problem(a, q);
  const size_t mn = static_cast<size_t>(a.m) * a.n;
  const T *src = a.src;
  T *A = a.ws + a.oA;
  for (size_t idx = static_cast<size_t>(blockIdx.x) * kTPB + threadIdx.x; idx < mn;
       idx += static_cast<size_t>(gridDim.x) * kTPB) {
    const size_t i = idx / a.n, c = idx % a.n;
    A[idx] = a.rowmaj ? src[idx] : src[c * a.m + i];
  }
}

// Sinkhorn-Knopp on A.^2 (equil_helper.h:140-164, all 50 passes), passes [p0, p0 + np) of them.  grid: problems
template <typename T>
__global__ __launch_bounds__(kTPB) void many_sk_kernel(ManyArgs<T> a, int p0, int np) {
  __shared__ T part[kTPB];
  const int q = blockIdx.x;
  many_problem(a, q);
  const int m = a.m, n = a.n;
  T *w = a.ws;
  const T *A = w + a.oA;
  T *d = w + a.oy[kD], *e = w + a.ox[kE];
  if (p0 == 0) {
    for (int i = threadIdx.x; i < m; i += kTPB) d[i] = 1;
    __syncthreads();
  }
  const T tm = static_cast<T>(m), tn = static_cast<T>(n), ce = a.ce, cd = a.cd;
  for (int p = p0; p < p0 + np; ++p) {
    col_dots<T, true>(A, n, m, n, [](int) { return 0; }, d, [&](int c, T s) { e[c] = tm / (s + ce); }, part);
    __syncthreads();
    row_dots<T, true>(A, n, m, [&](int) { return n; }, e, [&](int i, T s) { d[i] = tn / (s + cd); });
    __syncthreads();
  }
}

// MatrixDense::Equil's closing steps (matrix_dense.cpp:176-192): d, e <- sqrt; A <- diag(d) A diag(e) (as the
// sign-bit round trip leaves it, sign(a) sqrt(a^2)); A, d, e normalised by ||A||_F / sqrt(min(m, n)).  grid: problems
template <typename T>
__global__ __launch_bounds__(kTPB) void many_scale_kernel(ManyArgs<T> a) {
  __shared__ double red[1 * (kWaves + 1)];
  const int q = blockIdx.x;
  many_problem(a, q);
  const int m = a.m, n = a.n;
  T *w = a.ws;
  T *A = w + a.oA, *d = w + a.oy[kD], *e = w + a.ox[kE];
  for (int i = threadIdx.x; i < m; i += kTPB) d[i] = dev::Sqrt(d[i]);
  for (int j = threadIdx.x; j < n; j += kTPB) e[j] = dev::Sqrt(e[j]);
  __syncthreads();
  const size_t mn = static_cast<size_t>(m) * n;
  double fro[1] = {0};
  for (size_t idx = threadIdx.x; idx < mn; idx += kTPB) {
    const size_t i = idx / n, c = idx % n;
    const T v0 = A[idx];
    T v = static_cast<T>(1 - 2 * (v0 < 0)) * dev::Sqrt(v0 * v0);
    v *= d[i] * e[c];
    A[idx] = v;
    fro[0] += static_cast<double>(v) * v;
  }
  wg_sum<1>(fro, red);
  const T normA = static_cast<T>(sqrt(fro[0])) / dev::Sqrt(static_cast<T>(m < n ? m : n));
  const T inv = static_cast<T>(1) / normA;
  for (size_t idx = threadIdx.x; idx < mn; idx += kTPB) A[idx] *= inv;
  const T invs = static_cast<T>(1) / dev::Sqrt(normA);
  for (int i = threadIdx.x; i < m; i += kTPB) d[i] *= invs;
  for (int j = threadIdx.x; j < n; j += kTPB) e[j] *= invs;
}

// Norm2Est (equil_helper.h:107-135) on the equilibrated A: power iterations [it0, it0 + nit), state in ManyState.
// grid: problems
template <typename T>
__global__ __launch_bounds__(kTPB) void many_normest_kernel(ManyArgs<T> a, int it0, int nit) {
  __shared__ double red[2 * (kWaves + 1)];
  __shared__ T part[kTPB];
  const int q = blockIdx.x;
  ManyState<T> &st = a.st[q];
  if (it0 > 0 && st.ne_done) return;
  many_problem(a, q);
  const int m = a.m, n = a.n;
  T *w = a.ws;
  const T *A = w + a.oA;
  T *x = w + a.ox[kXtemp], *Sx = w + a.oy[kYtemp];
  T est = 0;
  int it = 0;
  if (it0 == 0) {
    for (int j = threadIdx.x; j < n; j += kTPB) x[j] = a.rnd[j];
    __syncthreads();
  } else {
    est = st.ne_est;
    it = st.ne_iter;
  }
  const T kTol = static_cast<T>(1e-4);
  bool done = false;
  for (int r = 0; r < nit && it < 50; ++r) {
    const T last = est;
    row_dots<T, false>(A, n, m, [&](int) { return n; }, x, [&](int i, T s) { Sx[i] = s; });
    __syncthreads();
    col_dots<T, false>(A, n, m, n, [](int) { return 0; }, Sx, [&](int c, T s) { x[c] = s; }, part);
    __syncthreads();
    double s2[2] = {0, 0};
    for (int j = threadIdx.x; j < n; j += kTPB) s2[0] += static_cast<double>(x[j]) * x[j];
    for (int i = threadIdx.x; i < m; i += kTPB) s2[1] += static_cast<double>(Sx[i]) * Sx[i];
    wg_sum<2>(s2, red);
    const T normx = static_cast<T>(sqrt(s2[0])), normSx = static_cast<T>(sqrt(s2[1]));
    const T sc = static_cast<T>(1) / normx;
    for (int j = threadIdx.x; j < n; j += kTPB) x[j] *= sc;
    est = normx / normSx;
    ++it;
    __syncthreads();
    if (dev::Abs(last - est) < kTol * est) { done = true; break; }
  }
  if (threadIdx.x == 0) {
    st.ne_est = est;
    st.ne_iter = it;
    st.ne_done = done || it >= 50;
    st.nrmA = est;
  }
}

// Lower triangle of the Gram matrix, A^T A (m > n) or A A^T (m <= n), into W: one 64 x 64 tile per workgroup,
// 4 x 4 per thread, summed over the long dimension in order.  grid (lower tiles, problems)
template <typename T>
__global__ __launch_bounds__(kTPB) void many_gram_kernel(ManyArgs<T> a) {
  const int q = blockIdx.y;
  many_problem(a, q);
  const int k = a.k, n = a.n;
  const int t = blockIdx.x;
  // the grid covers the largest problem of the launch: a tile past this problem's own count has nothing to do (the
  // kernel has no barrier, and the test is uniform over the workgroup)
  const int nb = (k + 63) / 64;
  if (t >= nb * (nb + 1) / 2) return;
  int bi = 0;
  while ((bi + 1) * (bi + 2) / 2 <= t) ++bi;
  const int bj = t - bi * (bi + 1) / 2;
  T *w = a.ws;
  const T *A = w + a.oA;
  T *G = w + a.oW;
  const int i0 = bi * 64 + (threadIdx.x / 16) * 4, j0 = bj * 64 + (threadIdx.x % 16) * 4;
  const int R = a.tall ? a.m : a.n;
  // element (r, i) of the factor whose Gram is formed: A[r][i] (tall) or A[i][r] (wide)
  const size_t si = a.tall ? 1 : static_cast<size_t>(n), sr = a.tall ? static_cast<size_t>(n) : 1;
  T acc[4][4] = {};
  for (int r = 0; r < R; ++r) {
    T u[4], v[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      u[p] = i0 + p < k ? A[r * sr + (i0 + p) * si] : static_cast<T>(0);
      v[p] = j0 + p < k ? A[r * sr + (j0 + p) * si] : static_cast<T>(0);
    }
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int s = 0; s < 4; ++s) acc[p][s] += u[p] * v[s];
  }
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int s = 0; s < 4; ++s)
      if (i0 + p < k && j0 + s <= i0 + p) G[static_cast<size_t>(i0 + p) * k + j0 + s] = acc[p][s];
}

// I + G = L L^T (the left-looking row Cholesky of gsl_linalg.h:12-55, diagonal sums in fp64), then W = L^-1 in place
// (column by column from the right, as LAPACK's trti2).  Lower triangles only.  grid: problems
template <typename T>
__global__ __launch_bounds__(kTPB) void many_factor_kernel(ManyArgs<T> a) {
  __shared__ T bc;
  const int q = blockIdx.x;
  many_problem(a, q);
  const int k = a.k;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  T *w = a.ws;
  T *L = w + a.oW, *tmp = w + a.oT;
  for (int j = 0; j < k; ++j) {
    const T *lj = L + static_cast<size_t>(j) * k;
    if (wv == 0) {
      double s = 0;
      for (int p = lane; p < j; p += 64) s += static_cast<double>(lj[p]) * lj[p];
      s = dev::wave_sum(s);
      if (lane == 0) {
        const double djj = static_cast<double>(static_cast<T>(lj[j] + static_cast<T>(1))) - s;
        const T ljj = static_cast<T>(sqrt(djj));
        L[static_cast<size_t>(j) * k + j] = ljj;
        bc = ljj;
      }
    }
    __syncthreads();
    const T ljj = bc;
    for (int i = j + 1 + wv; i < k; i += kWaves) {
      T *li = L + static_cast<size_t>(i) * k;
      T acc = 0;
      for (int p = lane; p < j; p += 64) acc += li[p] * lj[p];
      acc = dev::wave_sum(acc);
      if (lane == 0) li[j] = (li[j] - acc) / ljj;
    }
    __syncthreads();
  }
  for (int j = k - 1; j >= 0; --j) {
    for (int p = j + 1 + threadIdx.x; p < k; p += kTPB) tmp[p] = L[static_cast<size_t>(p) * k + j];
    if (threadIdx.x == 0) {
      const T wjj = static_cast<T>(1) / L[static_cast<size_t>(j) * k + j];
      L[static_cast<size_t>(j) * k + j] = wjj;
      bc = -wjj;
    }
    __syncthreads();
    const T ajj = bc;
    for (int i = j + 1 + wv; i < k; i += kWaves) {
      const T *wi = L + static_cast<size_t>(i) * k;
      T acc = 0;
      for (int p = j + 1 + lane; p <= i; p += 64) acc += wi[p] * tmp[p];
      acc = dev::wave_sum(acc);
      if (lane == 0) L[static_cast<size_t>(i) * k + j] = ajj * acc;
    }
    __syncthreads();
  }
}

// ---- the ADMM loop ----------------------------------------------------------------------------------

// At most `iters` iterations of every live problem (PogsImplementation::Solve, pogs.cpp:252-469, in its order; the
// direct projector of projector_direct_dense.cpp:87-175 with the factor's inverse), then, for a problem that stops,
// optval and the un-scaled outputs (pogs.cpp:473-518).  grid: problems
template <typename T>
__global__ __launch_bounds__(kTPB) void many_loop_kernel(ManyArgs<T> a, int iters) {
  __shared__ double red[6 * (kWaves + 1)];
  __shared__ T part[kTPB];
  const int q = blockIdx.x;
  if (a.st[q].stopped) return;
  const int bound = many_problem(a, q);
  iters = iters < bound ? iters : bound;
  const int m = a.m, n = a.n, k = a.k;
  T *w = a.ws;
  const T *A = w + a.oA, *W = w + a.oW;
  T *tv = w + a.oT;
  T *x = w + a.ox[kX], *xt = w + a.ox[kXt], *xprev = w + a.ox[kXprev], *x12 = w + a.ox[kX12];
  T *xtemp = w + a.ox[kXtemp], *xs = w + a.ox[kXs];
  const T *e = w + a.ox[kE];
  T *y = w + a.oy[kY], *yt = w + a.oy[kYt], *yprev = w + a.oy[kYprev], *y12 = w + a.oy[kY12];
  T *ytemp = w + a.oy[kYtemp], *ys = w + a.oy[kYs];
  const T *d = w + a.oy[kD];
  const ManyFn<T> F = a.fn[2 * q], G = a.fn[2 * q + 1];
  const T nrmA = a.st[q].nrmA;
  // every thread runs the control on the same (broadcast) sums and makes the same decisions; thread 0 stores it
  AdmmControl<T> c = a.ctl[q];
  T rho = c.rho;
  const T alpha = c.alpha(), oma = static_cast<T>(1) - alpha;
  double S[kNumSlots];
  for (int i = 0; i < kNumSlots; ++i) S[i] = 0;
  auto all_cols = [](int) { return 0; };
  auto full_row = [&](int) { return n; };
  for (int it = 0; it < iters; ++it) {
    // zprev = z; z -= zt; z12 = prox(z); z -= z12; the pre-projection sums (pogs.cpp:254-273)
    double s6[6] = {0, 0, 0, 0, 0, 0};
    for (int j = threadIdx.x; j < n; j += kTPB) {
      const T xp = x[j];
      xprev[j] = xp;
      const T v = xp - xt[j];
      const Coef<T> g = coef(G, j, e[j], false);
      const T h = dev::ProxEval(g.h, g.a, g.b, g.c, g.d, g.e, v, rho);
      x12[j] = h;
      const T r = v - h;
      x[j] = r;
      s6[0] += static_cast<double>(r) * h;
      s6[1] += static_cast<double>(r) * r;
      s6[2] += static_cast<double>(h) * h;
    }
    for (int i = threadIdx.x; i < m; i += kTPB) {
      const T yp = y[i];
      yprev[i] = yp;
      const T v = yp - yt[i];
      const Coef<T> f = coef(F, i, d[i], true);
      const T h = dev::ProxEval(f.h, f.a, f.b, f.c, f.d, f.e, v, rho);
      y12[i] = h;
      const T r = v - h;
      y[i] = r;
      s6[3] += static_cast<double>(r) * h;
      s6[4] += static_cast<double>(r) * r;
      s6[5] += static_cast<double>(h) * h;
    }
    wg_sum<6>(s6, red);
    S[kGapX] = s6[0]; S[kWX2] = s6[1]; S[kHX2] = s6[2];
    S[kGapY] = s6[3]; S[kWY2] = s6[4]; S[kHY2] = s6[5];
    c.set_pre(S);
    // ztemp = zt + alpha z12 + (1 - alpha) zprev (pogs.cpp:276-278)
    for (int j = threadIdx.x; j < n; j += kTPB) xtemp[j] = (xt[j] + alpha * x12[j]) + oma * xprev[j];
    for (int i = threadIdx.x; i < m; i += kTPB) ytemp[i] = (yt[i] + alpha * y12[i]) + oma * yprev[i];
    __syncthreads();
    // projection of ztemp onto y = A x (projector_direct_dense.cpp:122-135), (I + G)^-1 = W^T W
    if (a.tall) {
      col_dots<T, false>(A, n, m, n, all_cols, ytemp, [&](int j, T s) { xs[j] = xtemp[j] + s; }, part);
      __syncthreads();
      row_dots<T, false>(W, k, k, [](int i) { return i + 1; }, xs, [&](int i, T s) { tv[i] = s; });
      __syncthreads();
      col_dots<T, false>(W, k, k, k, [](int j) { return j; }, tv, [&](int j, T s) { x[j] = s; }, part);
      __syncthreads();
      row_dots<T, false>(A, n, m, full_row, x, [&](int i, T s) { y[i] = s; });
      __syncthreads();
    } else {
      row_dots<T, false>(A, n, m, full_row, xtemp, [&](int i, T s) { ys[i] = s - ytemp[i]; });
      __syncthreads();
      row_dots<T, false>(W, k, k, [](int i) { return i + 1; }, ys, [&](int i, T s) { tv[i] = s; });
      __syncthreads();
      col_dots<T, false>(W, k, k, k, [](int j) { return j; }, tv, [&](int j, T s) { ys[j] = s; }, part);
      __syncthreads();
      col_dots<T, false>(A, n, m, n, all_cols, ys, [&](int j, T s) { x[j] = xtemp[j] - s; }, part);
      for (int i = threadIdx.x; i < m; i += kTPB) y[i] = ys[i] + ytemp[i];
      __syncthreads();
    }
    // approximate residuals (pogs.cpp:342-348)
    double s4[4] = {0, 0, 0, 0};
    for (int j = threadIdx.x; j < n; j += kTPB) {
      const T u = xprev[j] - x[j], v = x12[j] - x[j];
      s4[0] += static_cast<double>(u) * u;
      s4[1] += static_cast<double>(v) * v;
    }
    for (int i = threadIdx.x; i < m; i += kTPB) {
      const T u = yprev[i] - y[i], v = y12[i] - y[i];
      s4[2] += static_cast<double>(u) * u;
      s4[3] += static_cast<double>(v) * v;
    }
    wg_sum<4>(s4, red);
    S[kDXprev2] = s4[0]; S[kDX12] = s4[1]; S[kDYprev2] = s4[2]; S[kDY12] = s4[3];
    const bool exact = c.set_approx(S, nrmA);
    if (exact) {
      // exact residuals (pogs.cpp:352-373)
      row_dots<T, false>(A, n, m, full_row, x12, [&](int i, T s) { ytemp[i] = s - y12[i]; });
      __syncthreads();
      double r2[1] = {0};
      for (int i = threadIdx.x; i < m; i += kTPB) r2[0] += static_cast<double>(ytemp[i]) * ytemp[i];
      wg_sum<1>(r2, red);
      for (int i = threadIdx.x; i < m; i += kTPB) ytemp[i] = (y12[i] + yt[i]) - yprev[i];
      for (int j = threadIdx.x; j < n; j += kTPB) xtemp[j] = (x12[j] + xt[j]) - xprev[j];
      __syncthreads();
      col_dots<T, false>(A, n, m, n, all_cols, ytemp, [&](int j, T s) { xtemp[j] = xtemp[j] + s; }, part);
      __syncthreads();
      double s2[1] = {0};
      for (int j = threadIdx.x; j < n; j += kTPB) s2[0] += static_cast<double>(xtemp[j]) * xtemp[j];
      wg_sum<1>(s2, red);
      S[kExactR2] = r2[0];
      S[kExactS2] = s2[0];
      c.set_exact(S);
    }
    const bool stop = c.check_stop(exact);
    if (stop) {
      // optval = f(y12) + g(x12) (pogs.cpp:473), then the un-scaled outputs (:510-518, 567-570)
      double fv[2] = {0, 0};
      for (int i = threadIdx.x; i < m; i += kTPB) {
        const Coef<T> f = coef(F, i, d[i], true);
        fv[0] += static_cast<double>(dev::FuncEval(f.h, f.a, f.b, f.c, f.d, f.e, y12[i]));
      }
      for (int j = threadIdx.x; j < n; j += kTPB) {
        const Coef<T> g = coef(G, j, e[j], false);
        fv[1] += static_cast<double>(dev::FuncEval(g.h, g.a, g.b, g.c, g.d, g.e, x12[j]));
      }
      wg_sum<2>(fv, red);
      const T nr = -rho;
      for (int i = threadIdx.x; i < m; i += kTPB) {
        a.lo[i] = (((yt[i] - yprev[i]) + y12[i]) * nr) * d[i];
        a.yo[i] = y12[i] / d[i];
      }
      for (int j = threadIdx.x; j < n; j += kTPB) {
        a.muo[j] = (((xt[j] - xprev[j]) + x12[j]) * nr) / e[j];
        a.xo[j] = x12[j] * e[j];
      }
      if (threadIdx.x == 0) {
        a.optval[q] = static_cast<double>(static_cast<T>(fv[0]) + static_cast<T>(fv[1]));
        a.iters[q] = c.k;
        a.status[q] = c.status();
        a.ctl[q] = c;
        a.st[q].stopped = 1;
        atomicAdd(a.done_count, 1u);
      }
      return;
    }
    const T scale = c.adapt();
    ++c.k;
    // zt += alpha z12 + (1 - alpha) zprev - z, then the rho change's rescaling (pogs.cpp:397-466)
    for (int j = threadIdx.x; j < n; j += kTPB) xt[j] = (((xt[j] + alpha * x12[j]) + oma * xprev[j]) - x[j]) * scale;
    for (int i = threadIdx.x; i < m; i += kTPB) yt[i] = (((yt[i] + alpha * y12[i]) + oma * yprev[i]) - y[i]) * scale;
    rho = c.rho;
    __syncthreads();
  }
  if (threadIdx.x == 0) a.ctl[q] = c;
}

// The start of a solve on a persistent handle, before its first loop launch: the problem is live again, and its
// iterate is the cold start (z = zt = 0: x, xt, y, yt are the vectors the loop reads before it writes them) or, where
// warm[q] is set (warm == nullptr: every problem cold), the reference's SetInitX + SetInitLambda (pogs.cpp:144-156)
// from the problem's kept un-scaled x and l (a.xo, a.lo): x = x0 / e, y = A x, t = l0 / d, xt = (-A^T t)(-1 / rho),
// yt = t (-1 / rho), with the rho of the control block this solve starts from.  The sums are row_dots / col_dots with
// the loop's maps.  grid: problems
template <typename T>
__global__ __launch_bounds__(kTPB) void many_begin_kernel(ManyArgs<T> a, const int *warm) {
  __shared__ T part[kTPB];
  const int q = blockIdx.x;
  many_problem(a, q);
  const int m = a.m, n = a.n;
  T *w = a.ws;
  const T *A = w + a.oA;
  T *x = w + a.ox[kX], *xt = w + a.ox[kXt], *y = w + a.oy[kY], *yt = w + a.oy[kYt], *ytemp = w + a.oy[kYtemp];
  const T *e = w + a.ox[kE], *d = w + a.oy[kD];
  if (threadIdx.x == 0) a.st[q].stopped = 0;
  if (!warm || !warm[q]) {
    for (int j = threadIdx.x; j < n; j += kTPB) { x[j] = 0; xt[j] = 0; }
    for (int i = threadIdx.x; i < m; i += kTPB) { y[i] = 0; yt[i] = 0; }
    return;
  }
  const T *x0 = a.xo, *l0 = a.lo;
  const T mr = static_cast<T>(-1) / a.ctl[q].rho;
  for (int j = threadIdx.x; j < n; j += kTPB) x[j] = x0[j] / e[j];
  for (int i = threadIdx.x; i < m; i += kTPB) ytemp[i] = l0[i] / d[i];
  __syncthreads();
  row_dots<T, false>(A, n, m, [&](int) { return n; }, x, [&](int i, T s) { y[i] = s; });
  col_dots<T, false>(A, n, m, n, [](int) { return 0; }, ytemp, [&](int j, T s) { xt[j] = (-s) * mr; }, part);
  for (int i = threadIdx.x; i < m; i += kTPB) yt[i] = ytemp[i] * mr;
}

}  // namespace
}  // namespace pogs_amd

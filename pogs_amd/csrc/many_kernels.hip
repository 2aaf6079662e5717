// Many small dense problems, each with its own matrix (PogsAmdSolveManyFn, include/pogs_amd.h).
//
// One workgroup owns one problem from setup to epilogue: it copies and equilibrates its A_j, estimates its norm,
// factors I + A^T A (m > n) or I + A A^T (m <= n), inverts the Cholesky factor (W = L^-1), and runs the two-pass
// ADMM iteration of pogs.cpp with the stopping rule and adaptive rho of AdmmControl (engine.h) on the device.  Only
// the Gram matrix is formed by several workgroups per problem (one 64 x 64 tile each).  Problems never talk to each
// other, so there is no host poll per iteration: a loop launch advances every live problem by at most a fixed number
// of iterations, keeps its state in device memory, and the host reads back one done-count per launch.
//
// Every sum inside a problem runs in a fixed order that depends on (m, n) alone (fixed thread -> element maps,
// fixed butterflies, partials combined in index order), and a problem's arithmetic never looks at its index, the
// chunk or the other problems: its bytes are its own.
//
// The ragged entries (PogsAmdSolveManyRaggedFn / PogsAmdManyCreateRagged) give every problem its own shape: a table
// with one row per problem (ManyProb) tells each workgroup its (m, n) and where its data lives, and many_problem(),
// called once at the top of every kernel, turns the kernel's arguments into that problem's; the code below it is the
// same for both layouts.
//
// The persistent handle (PogsAmdManyCreate / PogsAmdManySolveFn) runs the same setup once, keeps all k problems
// resident and opens every solve with many_begin_kernel: cold, or warm from a problem's kept x, l and rho.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "many_kernels.h"
#include "prox.h"
#include "reduce.h"

namespace pogs_amd {

void rand_uniform_host(float *x, size_t n);    // abi.hip: the Norm2Est start vector (gsl_rand.h:8-16)
void rand_uniform_host(double *x, size_t n);

namespace {

constexpr int kTPB = 256;
constexpr int kWaves = kTPB / 64;
constexpr int kMaxIterPerLaunch = 64;
// Work of one workgroup in one launch is bounded by about this many bytes streamed (the Sinkhorn-Knopp passes, the
// power iterations and the ADMM iterations are cut into launches by it), so that no launch runs long at the edge of
// the envelope (16384 x 512 fp64 = 64 MB per pass over A).
constexpr double kLaunchBytes = 256.0 * (1 << 20);

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

// x-sized and y-sized work vectors of a problem (z = [x | y] of pogs.cpp:129-138, its copies, the scalings)
enum XVec : int { kX = 0, kXt, kXprev, kX12, kXtemp, kE, kXs, kNumX };
enum YVec : int { kY = 0, kYt, kYprev, kY12, kYtemp, kD, kYs, kNumY };

// One row of the ragged table (ManyArgs::prob): problem q's own shape, where it lives in every pool (element
// offsets from the pools' base pointers in ManyArgs), its Sinkhorn-Knopp regularisers and its iteration bound.
template <typename T>
struct ManyProb {
  int m, n;
  int ipl, pad;                  // ADMM iterations per loop launch (many_iters_per_launch of its shape)
  size_t ws, src, xo, yo;        // workspace; staged input; x-sized outputs (x, mu); y-sized outputs (y, l)
  T ce, cd;
};

template <typename T>
struct ManyArgs {
  int m, n, k, tall;
  size_t stride;                 // elements of T per problem in ws
  size_t oA, oW, oT, ox[kNumX], oy[kNumY];
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

// A problem's workspace layout from its shape alone (offsets in elements of T): every array starts on a multiple of
// 64 elements, and so does the next problem's workspace.
template <typename T>
__host__ __device__ __forceinline__ void many_offsets(ManyArgs<T> &a, int m, int n) {
  const int K = m < n ? m : n;
  const size_t mz = static_cast<size_t>(m), nz = static_cast<size_t>(n), Kz = static_cast<size_t>(K);
  const size_t rm = (mz + 63) / 64 * 64, rn = (nz + 63) / 64 * 64;
  a.m = m; a.n = n; a.k = K; a.tall = m > n;
  size_t off = 0;
  a.oA = off; off += (mz * nz + 63) / 64 * 64;
  a.oW = off; off += (Kz * Kz + 63) / 64 * 64;
  a.oT = off; off += (Kz + 63) / 64 * 64;
  for (int v = 0; v < kNumX; ++v) { a.ox[v] = off; off += rn; }
  for (int v = 0; v < kNumY; ++v) { a.oy[v] = off; off += rm; }
  a.stride = off;
}

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

// ---- host driver ------------------------------------------------------------------------------------

size_t workspace_cap_bytes(int device) {
  const char *env = std::getenv("POGS_AMD_MANY_WORKSPACE_MB");
  if (env && env[0]) {
    const double mb = std::atof(env);
    if (mb > 0) return static_cast<size_t>(mb * (1 << 20));
  }
  size_t total = 0;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess) total = prop.totalGlobalMem;
  return total ? total / 8 : (size_t(4) << 30);
}

// The shape fields of ManyArgs: the problem's workspace layout (offsets in elements of T) and the Sinkhorn-Knopp
// regularisers (equil_helper.h:152-153, 159-160).
template <typename T>
void many_layout(ManyArgs<T> &a, int ord, size_t m_, size_t n_) {
  many_offsets(a, static_cast<int>(m_), static_cast<int>(n_));
  a.rowmaj = ord == ROW_MAJ;
  a.ce = static_cast<T>(1e-4) * static_cast<T>(m_ + n_) / static_cast<T>(m_);
  a.cd = static_cast<T>(1e-4) * static_cast<T>(m_ + n_) / static_cast<T>(n_);
}

// ADMM iterations per loop launch: kMaxIterPerLaunch, fewer where an iteration streams much (kLaunchBytes).
template <typename T>
int many_iters_per_launch(size_t mn, int K) {
  const double iter_bytes = (2.0 * static_cast<double>(mn) + static_cast<double>(K) * K) * sizeof(T);
  return static_cast<int>(std::max(1.0, std::min<double>(kMaxIterPerLaunch, kLaunchBytes / iter_bytes)));
}

// The shapes of a call's k problems and where problem j starts in every packed array: rows (f, y, l), columns
// (g, x, mu), matrix elements (A) and workspace elements.  Uniform: one (m, n), problem j at j times the size,
// nothing stored per problem.  Ragged: the prefix sums of the k shapes.
template <typename T>
struct ManyShapes {
  int k = 0;
  bool ragged = false;
  size_t m0 = 0, n0 = 0, stride0 = 0;          // uniform: the shape and its workspace stride; ragged: the largest m, n
  std::vector<size_t> mv, nv, r0, c0, e0, w0;  // ragged: the shapes and the k + 1 prefix sums

  void set_uniform(int kk, size_t m, size_t n) {
    ManyArgs<T> a{};
    many_offsets(a, static_cast<int>(m), static_cast<int>(n));
    k = kk; ragged = false; m0 = m; n0 = n; stride0 = a.stride;
  }
  void set_ragged(int kk, const size_t *m, const size_t *n) {
    const size_t kz = static_cast<size_t>(kk);
    k = kk; ragged = true; m0 = 0; n0 = 0;
    mv.assign(m, m + kz); nv.assign(n, n + kz);
    r0.assign(kz + 1, 0); c0.assign(kz + 1, 0); e0.assign(kz + 1, 0); w0.assign(kz + 1, 0);
    for (size_t j = 0; j < kz; ++j) {
      ManyArgs<T> a{};
      many_offsets(a, static_cast<int>(m[j]), static_cast<int>(n[j]));
      r0[j + 1] = r0[j] + m[j]; c0[j + 1] = c0[j] + n[j]; e0[j + 1] = e0[j] + m[j] * n[j]; w0[j + 1] = w0[j] + a.stride;
      m0 = std::max(m0, m[j]); n0 = std::max(n0, n[j]);
    }
  }
  size_t m(size_t j) const { return ragged ? mv[j] : m0; }
  size_t n(size_t j) const { return ragged ? nv[j] : n0; }
  size_t row0(size_t j) const { return ragged ? r0[j] : j * m0; }
  size_t col0(size_t j) const { return ragged ? c0[j] : j * n0; }
  size_t el0(size_t j) const { return ragged ? e0[j] : j * m0 * n0; }
  size_t ws0(size_t j) const { return ragged ? w0[j] : j * stride0; }
  // the extent of problems [j0, j0 + cnt) in each packed array
  size_t rows(size_t j0, size_t cnt) const { return row0(j0 + cnt) - row0(j0); }
  size_t cols(size_t j0, size_t cnt) const { return col0(j0 + cnt) - col0(j0); }
  size_t els(size_t j0, size_t cnt) const { return el0(j0 + cnt) - el0(j0); }
  size_t wss(size_t j0, size_t cnt) const { return ws0(j0 + cnt) - ws0(j0); }
  // the rows of the ragged table for problems [j0, j0 + cnt), offsets counted from problem `base`
  void table(std::vector<ManyProb<T>> &t, size_t j0, size_t cnt, size_t base) const {
    t.resize(cnt);
    for (size_t q = 0; q < cnt; ++q) {
      const size_t j = j0 + q, mj = mv[j], nj = nv[j];
      ManyProb<T> &p = t[q];
      p.m = static_cast<int>(mj); p.n = static_cast<int>(nj);
      p.ipl = many_iters_per_launch<T>(mj * nj, static_cast<int>(std::min(mj, nj)));
      p.pad = 0;
      p.ws = w0[j] - w0[base]; p.src = e0[j] - e0[base]; p.xo = c0[j] - c0[base]; p.yo = r0[j] - r0[base];
      p.ce = static_cast<T>(1e-4) * static_cast<T>(mj + nj) / static_cast<T>(mj);
      p.cd = static_cast<T>(1e-4) * static_cast<T>(mj + nj) / static_cast<T>(nj);
    }
  }
};

// What the launches of problems [j0, j0 + cnt) are sized by: the largest matrix and the largest Gram order among
// them, the fewest and the most ADMM iterations per loop launch, and their workspace extent.
struct ManyExtent {
  size_t mn_max = 0, ws_elems = 0;
  int K_max = 0, ipl_min = kMaxIterPerLaunch, ipl_max = 1;
};
template <typename T>
ManyExtent many_extent(const ManyShapes<T> &sh, size_t j0, size_t cnt) {
  ManyExtent x;
  x.ws_elems = sh.wss(j0, cnt);
  for (size_t j = j0; j < j0 + (sh.ragged ? cnt : 1); ++j) {
    const size_t mn = sh.m(j) * sh.n(j);
    const int K = static_cast<int>(std::min(sh.m(j), sh.n(j)));
    const int ipl = many_iters_per_launch<T>(mn, K);
    x.mn_max = std::max(x.mn_max, mn);
    x.K_max = std::max(x.K_max, K);
    x.ipl_min = std::min(x.ipl_min, ipl);
    x.ipl_max = std::max(x.ipl_max, ipl);
  }
  return x;
}

// Problems packed into chunks in order: a chunk takes problems while their bytes (per(j)) fit under cap and their
// count under max_cnt, and holds at least one.  Returns the chunk starts and k.
template <typename Per>
std::vector<size_t> many_chunks(size_t k, size_t cap, size_t max_cnt, Per per) {
  std::vector<size_t> starts{0};
  size_t used = 0, cnt = 0;
  for (size_t j = 0; j < k; ++j) {
    const size_t b = per(j);
    if (cnt > 0 && (used + b > cap || cnt >= max_cnt)) {
      starts.push_back(j);
      used = 0;
      cnt = 0;
    }
    used += b;
    ++cnt;
  }
  starts.push_back(k);
  return starts;
}

// The Norm2Est start vector (n values) into rnd.
template <typename T>
void many_start_vector(T *rnd, size_t n, hipStream_t s) {
  std::vector<T> r(n);
  rand_uniform_host(r.data(), n);
  POGS_HIP_CHECK(hipMemcpyAsync(rnd, r.data(), n * sizeof(T), hipMemcpyHostToDevice, s));
  POGS_HIP_CHECK(hipStreamSynchronize(s));
}

// The setup of the cnt problems of a chunk (a: many_layout's fields, ws, st, src and rnd set): zero workspaces and
// states, then copy, all 50 Sinkhorn-Knopp passes, scale, norm estimate, Gram tiles, factor and W = L^-1.  Returns the
// number of launches.  The solve and PogsAmdManySetupCheck both run this sequence.
// x: the problems' extent (many_extent); the launches are cut by the largest matrix and the Gram grid covers the
// largest order.  ws0: where the cnt workspaces start (a.ws for a uniform chunk).
template <typename T>
unsigned long long many_setup(const ManyArgs<T> &a, int cnt, const ManyExtent &x, T *ws0, hipStream_t s) {
  const size_t mn = x.mn_max;
  const int K = x.K_max;
  const double pass_bytes = 2.0 * static_cast<double>(mn) * sizeof(T);
  const int per_launch = static_cast<int>(std::max(1.0, std::min(50.0, kLaunchBytes / pass_bytes)));
  const int nb = (K + 63) / 64, ntiles = nb * (nb + 1) / 2;
  const int copy_blocks = static_cast<int>(std::min<size_t>(64, (mn + kTPB - 1) / kTPB));
  unsigned long long launches = 0;
  POGS_HIP_CHECK(hipMemsetAsync(a.st, 0, static_cast<size_t>(cnt) * sizeof(ManyState<T>), s));
  // zero work vectors: the cold start (z = zt = 0)
  POGS_HIP_CHECK(hipMemsetAsync(ws0, 0, x.ws_elems * sizeof(T), s));
  hipLaunchKernelGGL(many_copy_kernel<T>, dim3(copy_blocks, cnt), dim3(kTPB), 0, s, a);
  ++launches;
  for (int p0 = 0; p0 < 50; p0 += per_launch) {
    hipLaunchKernelGGL(many_sk_kernel<T>, dim3(cnt), dim3(kTPB), 0, s, a, p0, std::min(per_launch, 50 - p0));
    ++launches;
  }
  hipLaunchKernelGGL(many_scale_kernel<T>, dim3(cnt), dim3(kTPB), 0, s, a);
  ++launches;
  for (int i0 = 0; i0 < 50; i0 += per_launch) {
    hipLaunchKernelGGL(many_normest_kernel<T>, dim3(cnt), dim3(kTPB), 0, s, a, i0, std::min(per_launch, 50 - i0));
    ++launches;
  }
  hipLaunchKernelGGL(many_gram_kernel<T>, dim3(ntiles, cnt), dim3(kTPB), 0, s, a);
  hipLaunchKernelGGL(many_factor_kernel<T>, dim3(cnt), dim3(kTPB), 0, s, a);
  launches += 2;
  POGS_HIP_CHECK(hipGetLastError());
  return launches;
}

// PogsAmdManySetupCheck: many_setup on k problems in one chunk, then per problem A_eq, d, e, nrmA and W (K x K).
template <typename T>
void many_setup_check_t(int ord, int kk, size_t m_, size_t n_, const void *Ain, int mem, T *A_eq, T *d, T *e,
                        double *nrmA, T *W) {
  Ctx ctx;
  ctx.init(-1, 0);
  hipStream_t s = ctx.stream;
  const size_t mn = m_ * n_;
  ManyArgs<T> a{};
  many_layout(a, ord, m_, n_);
  const size_t K = static_cast<size_t>(a.k);
  DevBuf<T> ws(static_cast<size_t>(kk) * a.stride), stage, rnd(n_);
  DevBuf<ManyState<T>> st(kk);
  many_start_vector(rnd.p, n_, s);
  const T *src = static_cast<const T *>(Ain);
  if (mem == POGS_AMD_HOST) {
    stage.alloc(static_cast<size_t>(kk) * mn);
    POGS_HIP_CHECK(hipMemcpyAsync(stage.p, src, static_cast<size_t>(kk) * mn * sizeof(T), hipMemcpyHostToDevice, s));
    src = stage.p;
  }
  a.ws = ws.p; a.rnd = rnd.p; a.st = st.p; a.src = src;
  ManyShapes<T> sh;
  sh.set_uniform(kk, m_, n_);
  many_setup(a, kk, many_extent(sh, 0, kk), ws.p, s);
  std::vector<ManyState<T>> hst(kk);
  POGS_HIP_CHECK(hipMemcpyAsync(hst.data(), st.p, static_cast<size_t>(kk) * sizeof(ManyState<T>), hipMemcpyDeviceToHost,
                                s));
  for (int q = 0; q < kk; ++q) {
    const T *w = ws.p + static_cast<size_t>(q) * a.stride;
    auto d2h = [&](T *dst, size_t off, size_t len) {
      if (dst) POGS_HIP_CHECK(hipMemcpyAsync(dst + q * len, w + off, len * sizeof(T), hipMemcpyDeviceToHost, s));
    };
    d2h(A_eq, a.oA, mn);
    d2h(d, a.oy[kD], m_);
    d2h(e, a.ox[kE], n_);
    d2h(W, a.oW, K * K);
  }
  POGS_HIP_CHECK(hipStreamSynchronize(s));
  if (nrmA)
    for (int q = 0; q < kk; ++q) nrmA[q] = static_cast<double>(hst[q].nrmA);
}

// The functions of cnt problems on their way to the device: per-element fields packed into one upload (tpool, hpool),
// broadcast fields as values.  The host copies live here until the next run.
template <typename T>
struct ManyFnUpload {
  std::vector<T> tp;
  std::vector<int> hp;
  std::vector<ManyFn<T>> fh;
  void run(const FnHost *f, const FnHost *g, const ManyShapes<T> &sh, size_t j0, int cnt, T *tpool, int *hpool,
           ManyFn<T> *fnd, hipStream_t s) {
    tp.clear();
    hp.clear();
    fh.resize(2 * static_cast<size_t>(cnt));
    for (int q = 0; q < cnt; ++q) {
      for (int side = 0; side < 2; ++side) {
        const FnHost &fn = side == 0 ? f[j0 + q] : g[j0 + q];
        const size_t len = side == 0 ? sh.m(j0 + q) : sh.n(j0 + q);
        warn_negative_coeffs<T>(fn, len);
        ManyFn<T> &d = fh[2 * q + side];
        const void *ptr[5] = {fn.a, fn.b, fn.c, fn.d, fn.e};
        for (int fld = 0; fld < 5; ++fld) {
          d.v[fld] = static_cast<T>(fn.s0[fld]);
          d.p[fld] = nullptr;
          if (ptr[fld]) {
            d.p[fld] = tpool + tp.size();
            const T *src_f = static_cast<const T *>(ptr[fld]);
            tp.insert(tp.end(), src_f, src_f + len);
          }
        }
        d.h0 = fn.h0;
        d.h = nullptr;
        if (fn.h) {
          d.h = hpool + hp.size();
          hp.insert(hp.end(), fn.h, fn.h + len);
        }
      }
    }
    if (!tp.empty()) POGS_HIP_CHECK(hipMemcpyAsync(tpool, tp.data(), tp.size() * sizeof(T), hipMemcpyHostToDevice, s));
    if (!hp.empty()) POGS_HIP_CHECK(hipMemcpyAsync(hpool, hp.data(), hp.size() * sizeof(int), hipMemcpyHostToDevice, s));
    POGS_HIP_CHECK(hipMemcpyAsync(fnd, fh.data(), 2 * static_cast<size_t>(cnt) * sizeof(ManyFn<T>), hipMemcpyHostToDevice,
                                  s));
  }
};

// The loop of cnt problems (a.done_count zeroed on the stream before): every launch advances each live problem by at
// most its own iterations per launch (x.ipl_max is the launch's bound, a ragged problem's table row may lower it;
// x.ipl_min bounds the number of launches), and the host reads one done-count per launch.  Returns the number of
// launches.
template <typename T>
unsigned long long many_run_loop(const ManyArgs<T> &a, int cnt, const ManyExtent &x, unsigned max_iter,
                                 unsigned *hdone, hipStream_t s) {
  const unsigned long long max_launches = (max_iter + x.ipl_min - 1) / x.ipl_min + 1;
  unsigned long long nl = 0;
  for (;;) {
    hipLaunchKernelGGL(many_loop_kernel<T>, dim3(cnt), dim3(kTPB), 0, s, a, x.ipl_max);
    POGS_HIP_CHECK(hipGetLastError());
    ++nl;
    POGS_HIP_CHECK(hipMemcpyAsync(hdone, a.done_count, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    POGS_HIP_CHECK(hipStreamSynchronize(s));
    if (*hdone >= static_cast<unsigned>(cnt)) break;
    POGS_CHECK(nl < max_launches, "many-problem solve: a problem did not stop within max_iter iterations");
  }
  return nl;
}

// The one summary line of a call (verbose > 0).  head: what precedes "; status".
inline void many_print_summary(const char *head, int k, const unsigned *final_iter, const int *status, double t_setup,
                               double t_loop, double t_total, unsigned long long launches) {
  int counts[7] = {0, 0, 0, 0, 0, 0, 0};
  unsigned it_lo = ~0u, it_hi = 0;
  for (int q = 0; q < k; ++q) {
    const int st = status[q];
    ++counts[st >= 0 && st < 7 ? st : 6];
    it_lo = std::min(it_lo, final_iter[q]);
    it_hi = std::max(it_hi, final_iter[q]);
  }
  std::printf("%s; status", head);
  for (int st = 0; st < 7; ++st)
    if (counts[st]) std::printf(" %s: %d,", status_string(st), counts[st]);
  std::printf(" iterations %u..%u; setup %.3e s, loop %.3e s, total %.3e s; %llu launches\n", it_lo, it_hi, t_setup,
              t_loop, t_total, launches);
  std::fflush(stdout);
}

// "of 500 x 300" or, ragged, "of 310..700 x 300..300": the shapes in a summary line.
template <typename T>
void many_shape_text(char *buf, size_t len, const ManyShapes<T> &sh) {
  if (!sh.ragged) {
    std::snprintf(buf, len, "%zu x %zu", sh.m0, sh.n0);
    return;
  }
  std::snprintf(buf, len, "%zu..%zu x %zu..%zu", *std::min_element(sh.mv.begin(), sh.mv.end()), sh.m0,
                *std::min_element(sh.nv.begin(), sh.nv.end()), sh.n0);
}

// The one-shot solve of the sh.k problems, uniform or ragged, in chunks under the workspace cap.
template <typename T>
void solve_many_t(int ord, const ManyShapes<T> &sh, const void *Ain, int mem, int device, const FnHost *f,
                  const FnHost *g, const double *rho0, const SolveParams &p, const BatchOut &out) {
  const double t0 = wall_s();
  Ctx ctx;
  ctx.init(device, 0);
  hipStream_t s = ctx.stream;
  const size_t kz = static_cast<size_t>(sh.k);
  ManyArgs<T> a{};
  many_layout(a, ord, sh.m0, sh.n0);   // ragged: every kernel replaces the shape fields by the problem's own
  // per problem: workspace, staged input, outputs, coefficient arrays, control (and its row of the ragged table)
  auto per = [&](size_t j) {
    const size_t len = sh.m(j) + sh.n(j);
    return sizeof(T) * (sh.wss(j, 1) + (mem == POGS_AMD_HOST ? sh.els(j, 1) : 0) + 2 * len + 5 * len) +
           sizeof(int) * len + sizeof(AdmmControl<T>) + sizeof(ManyState<T>) + 64 +
           (sh.ragged ? sizeof(ManyProb<T>) : 0);
  };
  const std::vector<size_t> starts = many_chunks(kz, workspace_cap_bytes(ctx.device), kz, per);
  // every buffer holds the largest chunk
  size_t chunk = 0, ws_e = 0, st_e = 0, rows = 0, cols = 0;
  for (size_t c = 0; c + 1 < starts.size(); ++c) {
    const size_t j0 = starts[c], cnt = starts[c + 1] - j0;
    chunk = std::max(chunk, cnt);
    ws_e = std::max(ws_e, sh.wss(j0, cnt));
    st_e = std::max(st_e, sh.els(j0, cnt));
    rows = std::max(rows, sh.rows(j0, cnt));
    cols = std::max(cols, sh.cols(j0, cnt));
    if (!sh.ragged) break;   // uniform: the first chunk is the largest
  }

  DevBuf<T> ws(ws_e), stage, rnd(sh.n0);
  if (mem == POGS_AMD_HOST) stage.alloc(st_e);
  DevBuf<T> xo(cols), yo(rows), lo(rows), muo(cols);
  DevBuf<double> optv(chunk);
  DevBuf<unsigned> iters(chunk), done(1);
  DevBuf<int> stat(chunk);
  DevBuf<ManyFn<T>> fnd(2 * chunk);
  DevBuf<AdmmControl<T>> ctld(chunk);
  DevBuf<ManyState<T>> std_(chunk);
  DevBuf<T> tpool(5 * (rows + cols) + 1);
  DevBuf<int> hpool(rows + cols + 1);
  DevBuf<ManyProb<T>> probd;
  if (sh.ragged) probd.alloc(chunk);
  PinnedBuf<unsigned> hdone(1);
  // the start vector of the widest problem: a narrower one reads its first n values, which are what it gets alone
  many_start_vector(rnd.p, sh.n0, s);
  a.ws = ws.p; a.rnd = rnd.p; a.fn = fnd.p; a.ctl = ctld.p; a.st = std_.p; a.done_count = done.p;
  a.xo = xo.p; a.yo = yo.p; a.lo = lo.p; a.muo = muo.p; a.optval = optv.p; a.iters = iters.p; a.status = stat.p;
  a.prob = probd.p;

  ManyFnUpload<T> up;
  std::vector<AdmmControl<T>> ch(chunk);
  std::vector<ManyProb<T>> tab;
  unsigned long long launches = 0;
  double t_setup = 0, t_loop = 0;
  for (size_t c = 0; c + 1 < starts.size(); ++c) {
    const size_t j0 = starts[c];
    const int cnt = static_cast<int>(starts[c + 1] - j0);
    const ManyExtent ext = many_extent(sh, j0, cnt);
    const double tc0 = wall_s();
    const T *src = static_cast<const T *>(Ain) + sh.el0(j0);
    if (mem == POGS_AMD_HOST) {
      POGS_HIP_CHECK(hipMemcpyAsync(stage.p, src, sh.els(j0, cnt) * sizeof(T), hipMemcpyHostToDevice, s));
      src = stage.p;
    }
    a.src = src;
    if (sh.ragged) {
      sh.table(tab, j0, cnt, j0);
      POGS_HIP_CHECK(hipMemcpyAsync(probd.p, tab.data(), tab.size() * sizeof(ManyProb<T>), hipMemcpyHostToDevice, s));
    }
    up.run(f, g, sh, j0, cnt, tpool.p, hpool.p, fnd.p, s);
    for (int q = 0; q < cnt; ++q)
      ch[q] = make_admm_control<T>(p, rho0 ? rho0[j0 + q] : 1.0, sh.m(j0 + q), sh.n(j0 + q));
    POGS_HIP_CHECK(hipMemcpyAsync(ctld.p, ch.data(), static_cast<size_t>(cnt) * sizeof(AdmmControl<T>),
                                  hipMemcpyHostToDevice, s));
    POGS_HIP_CHECK(hipMemsetAsync(done.p, 0, sizeof(unsigned), s));
    launches += many_setup(a, cnt, ext, ws.p, s);
    ctx.sync();
    const double tc1 = wall_s();
    t_setup += tc1 - tc0;
    // the loop: every launch advances each live problem by at most its iterations per launch
    launches += many_run_loop(a, cnt, ext, p.max_iter, hdone.p, s);
    t_loop += wall_s() - tc1;
    // outputs of the chunk
    auto d2h = [&](void *dst, const void *srcd, size_t bytes) {
      POGS_HIP_CHECK(hipMemcpyAsync(dst, srcd, bytes, hipMemcpyDeviceToHost, s));
    };
    const size_t xb = sh.cols(j0, cnt) * sizeof(T), yb = sh.rows(j0, cnt) * sizeof(T);
    d2h(static_cast<T *>(out.x) + sh.col0(j0), xo.p, xb);
    if (out.y) d2h(static_cast<T *>(out.y) + sh.row0(j0), yo.p, yb);
    if (out.l) d2h(static_cast<T *>(out.l) + sh.row0(j0), lo.p, yb);
    if (out.mu) d2h(static_cast<T *>(out.mu) + sh.col0(j0), muo.p, xb);
    if (out.optval) d2h(out.optval + j0, optv.p, cnt * sizeof(double));
    d2h(out.final_iter + j0, iters.p, cnt * sizeof(unsigned));
    d2h(out.status + j0, stat.p, cnt * sizeof(int));
    POGS_HIP_CHECK(hipStreamSynchronize(s));
  }
  if (p.verbose > 0) {
    char head[200], shape[96];
    many_shape_text(shape, sizeof(shape), sh);
    if (sh.ragged)
      std::snprintf(head, sizeof(head), "POGS-AMD many: %d ragged problems of %s (%s), %zu chunks of at most %zu", sh.k,
                    shape, sizeof(T) == 8 ? "fp64" : "fp32", starts.size() - 1, chunk);
    else
      std::snprintf(head, sizeof(head), "POGS-AMD many: %d problems of %s (%s), %zu per chunk", sh.k, shape,
                    sizeof(T) == 8 ? "fp64" : "fp32", chunk);
    many_print_summary(head, sh.k, out.final_iter, out.status, t_setup, t_loop, wall_s() - t0, launches);
  }
}


// The persistent handle (PogsAmdMany): setup once for all k problems in one resident workspace, then any number of
// solves, each opened by many_begin_kernel.  xo / lo double as the kept last solution the warm starts read.
template <typename T>
class ManyHandleT : public ManyHandle {
 public:
  ManyHandleT(int ord, ManyShapes<T> &&shapes, const void *Ain, int mem, int device)
      : sh_(std::move(shapes)), k_(sh_.k) {
    const double t0 = wall_s();
    ctx_.init(device, 0);
    hipStream_t s = ctx_.stream;
    many_layout(a_, ord, sh_.m0, sh_.n0);   // ragged: every kernel replaces the shape fields by the problem's own
    const size_t kz = static_cast<size_t>(k_);
    const size_t rows = sh_.rows(0, kz), cols = sh_.cols(0, kz), len = rows + cols, ws_e = sh_.wss(0, kz);
    std::memset(&info_, 0, sizeof(info_));
    info_.k = k_; info_.dtype = sizeof(T) == 8 ? POGS_AMD_F64 : POGS_AMD_F32; info_.m = sh_.m0; info_.n = sh_.n0;
    info_.resident_bytes = sizeof(T) * (ws_e + 2 * len + 5 * len + kz) + sizeof(int) * (len + 2 * kz) +
                           kz * (sizeof(double) + sizeof(unsigned) + 2 * sizeof(ManyFn<T>) + sizeof(AdmmControl<T>) +
                                 sizeof(ManyState<T>) + (sh_.ragged ? sizeof(ManyProb<T>) : 0));
    try {
      ws_.alloc(ws_e);
      xo_.alloc(cols); yo_.alloc(rows); lo_.alloc(rows); muo_.alloc(cols);
      optv_.alloc(kz); iters_.alloc(kz); stat_.alloc(kz); warm_.alloc(kz); done_.alloc(1);
      fnd_.alloc(2 * kz); ctld_.alloc(kz); st_.alloc(kz);
      tpool_.alloc(5 * len + 1); hpool_.alloc(len + 1);
      if (sh_.ragged) prob_.alloc(kz);
    } catch (const std::exception &e) {
      (void)hipGetLastError();
      char buf[512], shape[96];
      many_shape_text(shape, sizeof(shape), sh_);
      std::snprintf(buf, sizeof(buf),
                    "many-problem handle: the resident footprint of %d problems of %s (%.1f MB) cannot be "
                    "allocated; PogsAmdSolveManyFn solves them in chunks [%s]",
                    k_, shape, static_cast<double>(info_.resident_bytes) / (1 << 20), e.what());
      throw Error(buf);
    }
    hdone_.alloc(1);
    a_.ws = ws_.p; a_.fn = fnd_.p; a_.ctl = ctld_.p; a_.st = st_.p; a_.done_count = done_.p;
    a_.xo = xo_.p; a_.yo = yo_.p; a_.lo = lo_.p; a_.muo = muo_.p; a_.optval = optv_.p; a_.iters = iters_.p;
    a_.status = stat_.p;
    a_.prob = prob_.p;
    if (sh_.ragged) {
      // the handle's table counts every offset from problem 0: the pools' base pointers are the handle's buffers
      std::vector<ManyProb<T>> tab;
      sh_.table(tab, 0, kz, 0);
      POGS_HIP_CHECK(hipMemcpyAsync(prob_.p, tab.data(), kz * sizeof(ManyProb<T>), hipMemcpyHostToDevice, s));
      POGS_HIP_CHECK(hipStreamSynchronize(s));
    }
    // setup in chunks: a host A through a staging buffer under the workspace cap; a chunk is also the y extent of
    // the copy and Gram grids
    const size_t cap = mem == POGS_AMD_HOST ? workspace_cap_bytes(ctx_.device) : ~static_cast<size_t>(0);
    const std::vector<size_t> starts = many_chunks(kz, cap, 32768, [&](size_t j) {
      return mem == POGS_AMD_HOST ? sh_.els(j, 1) * sizeof(T) : static_cast<size_t>(0);
    });
    DevBuf<T> stage, rnd(sh_.n0);
    if (mem == POGS_AMD_HOST) {
      size_t st_e = 0;
      for (size_t c = 0; c + 1 < starts.size(); ++c) st_e = std::max(st_e, sh_.els(starts[c], starts[c + 1] - starts[c]));
      stage.alloc(st_e);
    }
    many_start_vector(rnd.p, sh_.n0, s);
    for (size_t ci = 0; ci + 1 < starts.size(); ++ci) {
      const size_t j0 = starts[ci];
      const int cnt = static_cast<int>(starts[ci + 1] - j0);
      const T *src = static_cast<const T *>(Ain) + sh_.el0(j0);
      if (mem == POGS_AMD_HOST) {
        POGS_HIP_CHECK(hipMemcpyAsync(stage.p, src, sh_.els(j0, cnt) * sizeof(T), hipMemcpyHostToDevice, s));
        src = stage.p;
      }
      // the chunk's problems are q = 0 .. cnt - 1 of this launch.  Uniform: the bases move to the chunk.  Ragged: the
      // table rows move, their offsets still count from problem 0, so ws stays, and src0 says that src points at the
      // chunk's first matrix
      ManyArgs<T> c = a_;
      c.st = st_.p + j0;
      c.rnd = rnd.p;
      if (sh_.ragged) {
        c.prob = prob_.p + j0;
        c.src = src;
        c.src0 = sh_.el0(j0);
      } else {
        c.ws = ws_.p + sh_.ws0(j0);
        c.src = src;
      }
      many_setup(c, cnt, many_extent(sh_, j0, cnt), ws_.p + sh_.ws0(j0), s);
    }
    ctx_.sync();
    ext_ = many_extent(sh_, 0, kz);
    last_status_.assign(kz, POGS_ERROR);
    last_rho_.assign(kz, 1.0);
    info_.setup_s = wall_s() - t0;
  }
  ~ManyHandleT() override { (void)hipStreamSynchronize(ctx_.stream); }

  int device() const override { return ctx_.device; }
  int count() const override { return k_; }
  PogsAmdManyInfo info() const override { return info_; }
  void shapes(size_t *m, size_t *n) const override {
    for (size_t j = 0; j < static_cast<size_t>(k_); ++j) {
      m[j] = sh_.m(j);
      n[j] = sh_.n(j);
    }
  }

  void solve(const FnHost *f, const FnHost *g, const ManyStart &sa, const SolveParams &p, const BatchOut &out) override {
    POGS_CHECK(out.x && out.final_iter && out.status, "many-problem handle: x, final_iter and status must not be NULL");
    POGS_CHECK(sa.start == POGS_AMD_MANY_COLD || sa.start == POGS_AMD_MANY_WARM_GIVEN ||
               sa.start == POGS_AMD_MANY_WARM_LAST, "many-problem handle: unknown start mode");
    POGS_CHECK(sa.start != POGS_AMD_MANY_WARM_GIVEN || (sa.x0 && sa.l0),
               "many-problem handle: a given warm start needs both x0 and l0 (pogs.cpp:159-179)");
    POGS_CHECK(sa.start != POGS_AMD_MANY_WARM_LAST || solved_,
               "many-problem handle: start = last before the handle's first solve");
    const double t0 = wall_s();
    hipStream_t s = ctx_.stream;
    const size_t kz = static_cast<size_t>(k_);
    const size_t xb = sh_.cols(0, kz) * sizeof(T), yb = sh_.rows(0, kz) * sizeof(T);
    up_.run(f, g, sh_, 0, k_, tpool_.p, hpool_.p, fnd_.p, s);
    ch_.resize(kz);
    hwarm_.resize(kz);
    for (size_t q = 0; q < kz; ++q) {
      const bool kept = last_status_[q] == POGS_SUCCESS || last_status_[q] == POGS_MAX_ITER;
      hwarm_[q] = sa.start == POGS_AMD_MANY_WARM_GIVEN || (sa.start == POGS_AMD_MANY_WARM_LAST && kept);
      double rho = sa.rho ? sa.rho[q] : 1.0;
      if (sa.start == POGS_AMD_MANY_WARM_LAST) rho = !kept ? 1.0 : sa.rho ? sa.rho[q] : last_rho_[q];
      ch_[q] = make_admm_control<T>(p, rho, sh_.m(q), sh_.n(q));
    }
    POGS_HIP_CHECK(hipMemcpyAsync(ctld_.p, ch_.data(), kz * sizeof(AdmmControl<T>), hipMemcpyHostToDevice, s));
    const int *warm = nullptr;
    if (sa.start != POGS_AMD_MANY_COLD) {
      POGS_HIP_CHECK(hipMemcpyAsync(warm_.p, hwarm_.data(), kz * sizeof(int), hipMemcpyHostToDevice, s));
      warm = warm_.p;
    }
    if (sa.start == POGS_AMD_MANY_WARM_GIVEN) {
      POGS_HIP_CHECK(hipMemcpyAsync(xo_.p, sa.x0, xb, hipMemcpyHostToDevice, s));
      POGS_HIP_CHECK(hipMemcpyAsync(lo_.p, sa.l0, yb, hipMemcpyHostToDevice, s));
    }
    POGS_HIP_CHECK(hipMemsetAsync(done_.p, 0, sizeof(unsigned), s));
    ctx_.sync();
    const double t1 = wall_s();
    hipLaunchKernelGGL(many_begin_kernel<T>, dim3(k_), dim3(kTPB), 0, s, a_, warm);
    POGS_HIP_CHECK(hipGetLastError());
    const unsigned long long launches = 1 + many_run_loop(a_, k_, ext_, p.max_iter, hdone_.p, s);
    const double t_loop = wall_s() - t1;
    auto d2h = [&](void *dst, const void *srcd, size_t bytes) {
      POGS_HIP_CHECK(hipMemcpyAsync(dst, srcd, bytes, hipMemcpyDeviceToHost, s));
    };
    d2h(out.x, xo_.p, xb);
    if (out.y) d2h(out.y, yo_.p, yb);
    if (out.l) d2h(out.l, lo_.p, yb);
    if (out.mu) d2h(out.mu, muo_.p, xb);
    if (out.optval) d2h(out.optval, optv_.p, kz * sizeof(double));
    d2h(out.final_iter, iters_.p, kz * sizeof(unsigned));
    d2h(out.status, stat_.p, kz * sizeof(int));
    d2h(ch_.data(), ctld_.p, kz * sizeof(AdmmControl<T>));
    POGS_HIP_CHECK(hipStreamSynchronize(s));
    unsigned long long piters = 0;
    for (size_t q = 0; q < kz; ++q) {
      last_status_[q] = out.status[q];
      last_rho_[q] = static_cast<double>(ch_[q].rho);
      if (sa.rho_final) sa.rho_final[q] = last_rho_[q];
      piters += out.final_iter[q] + 1ull;
    }
    solved_ = true;
    info_.loop_s = t_loop;
    info_.launches = launches;
    info_.problem_iters = piters;
    if (p.verbose > 0) {
      static const char *const kStart[3] = {"cold", "warm (given)", "warm (last)"};
      char head[240], shape[96];
      many_shape_text(shape, sizeof(shape), sh_);
      std::snprintf(head, sizeof(head), "POGS-AMD many handle: %d %sproblems of %s (%s), start %s", k_,
                    sh_.ragged ? "ragged " : "", shape, sizeof(T) == 8 ? "fp64" : "fp32", kStart[sa.start]);
      many_print_summary(head, k_, out.final_iter, out.status, 0.0, t_loop, wall_s() - t0, launches);
    }
  }

 private:
  ManyShapes<T> sh_;
  int k_;
  Ctx ctx_;
  ManyArgs<T> a_{};
  ManyExtent ext_;
  DevBuf<T> ws_, xo_, yo_, lo_, muo_, tpool_;
  DevBuf<ManyProb<T>> prob_;               // ragged: the table, offsets from problem 0
  DevBuf<double> optv_;
  DevBuf<unsigned> iters_, done_;
  DevBuf<int> stat_, hpool_, warm_;
  DevBuf<ManyFn<T>> fnd_;
  DevBuf<AdmmControl<T>> ctld_;
  DevBuf<ManyState<T>> st_;
  PinnedBuf<unsigned> hdone_;
  ManyFnUpload<T> up_;
  std::vector<AdmmControl<T>> ch_;
  std::vector<int> hwarm_, last_status_;   // each problem's status after the last solve (POGS_ERROR: none yet)
  std::vector<double> last_rho_;           // and the rho it stopped at
  bool solved_ = false;
  PogsAmdManyInfo info_;
};

}  // namespace

// The argument checks of every many-problem entry, `what` the prefix of their messages, in the order the entries
// report them: the call (dtype, k, ord, mem), then A and one shape's envelope.  A ragged entry checks its call the same
// way and words the rest per problem.
namespace {
void many_check_call(const std::string &what, int dtype, int ord, int k, int mem) {
  POGS_CHECK(dtype == POGS_AMD_F32 || dtype == POGS_AMD_F64, (what + ": unknown dtype").c_str());
  POGS_CHECK(k >= 1, (what + ": k must be >= 1").c_str());
  POGS_CHECK(ord == ROW_MAJ || ord == COL_MAJ, (what + ": unknown ord").c_str());
  POGS_CHECK(mem == POGS_AMD_HOST || mem == POGS_AMD_DEVICE, (what + ": unknown mem").c_str());
}

void many_check_uniform(const std::string &what, int dtype, int ord, int k, size_t m, size_t n, const void *A,
                        int mem) {
  many_check_call(what, dtype, ord, k, mem);
  POGS_CHECK(A != nullptr, (what + ": null A").c_str());
  POGS_CHECK(m >= 1 && n >= 1, (what + ": m and n must be >= 1").c_str());
  POGS_CHECK(std::min(m, n) <= POGS_AMD_MANY_MIN_DIM_MAX,
             (what + ": min(m, n) exceeds POGS_AMD_MANY_MIN_DIM_MAX").c_str());
  POGS_CHECK(std::max(m, n) <= POGS_AMD_MANY_MAX_DIM_MAX,
             (what + ": max(m, n) exceeds POGS_AMD_MANY_MAX_DIM_MAX").c_str());
}
}  // namespace

void many_check_args(int dtype, int ord, int k, size_t m, size_t n, const void *A, int mem) {
  many_check_uniform("many-problem solve", dtype, ord, k, m, n, A, mem);
}

void many_check_ragged(int dtype, int ord, int k, const size_t *m, const size_t *n, const void *A, int mem) {
  many_check_call("ragged many-problem solve", dtype, ord, k, mem);
  POGS_CHECK(m != nullptr && n != nullptr, "ragged many-problem solve: null m or n");
  POGS_CHECK(A != nullptr, "ragged many-problem solve: null A");
  for (int j = 0; j < k; ++j) {
    const char *why = m[j] < 1 || n[j] < 1 ? "m and n must be >= 1"
                      : std::min(m[j], n[j]) > POGS_AMD_MANY_MIN_DIM_MAX ? "min(m, n) exceeds POGS_AMD_MANY_MIN_DIM_MAX"
                      : std::max(m[j], n[j]) > POGS_AMD_MANY_MAX_DIM_MAX ? "max(m, n) exceeds POGS_AMD_MANY_MAX_DIM_MAX"
                                                                          : nullptr;
    if (why) {
      char buf[256];
      std::snprintf(buf, sizeof(buf), "ragged many-problem solve: problem %d of %d (m[%d] = %zu, n[%d] = %zu): %s", j, k,
                    j, m[j], j, n[j], why);
      throw Error(buf);
    }
  }
}

namespace {
template <typename T>
ManyHandle *many_new_handle(int ord, int k, size_t m, size_t n, const size_t *mv, const size_t *nv, const void *A,
                            int mem, int device) {
  ManyShapes<T> sh;
  if (mv) sh.set_ragged(k, mv, nv);
  else sh.set_uniform(k, m, n);
  return new ManyHandleT<T>(ord, std::move(sh), A, mem, device);
}
}  // namespace

ManyHandle *many_create(int dtype, int ord, int k, size_t m, size_t n, const void *A, int mem, int device) {
  many_check_args(dtype, ord, k, m, n, A, mem);
  DeviceGuard guard(device);
  if (dtype == POGS_AMD_F64) return many_new_handle<double>(ord, k, m, n, nullptr, nullptr, A, mem, device);
  return many_new_handle<float>(ord, k, m, n, nullptr, nullptr, A, mem, device);
}

ManyHandle *many_create_ragged(int dtype, int ord, int k, const size_t *m, const size_t *n, const void *A, int mem,
                               int device) {
  many_check_ragged(dtype, ord, k, m, n, A, mem);
  DeviceGuard guard(device);
  if (dtype == POGS_AMD_F64) return many_new_handle<double>(ord, k, 0, 0, m, n, A, mem, device);
  return many_new_handle<float>(ord, k, 0, 0, m, n, A, mem, device);
}

void solve_many_ragged(int dtype, int ord, int k, const size_t *m, const size_t *n, const void *A, int mem, int device,
                       const FnHost *f, const FnHost *g, const double *rho, const SolveParams &p, const BatchOut &out) {
  many_check_ragged(dtype, ord, k, m, n, A, mem);
  POGS_CHECK(out.x && out.final_iter && out.status,
             "ragged many-problem solve: x, final_iter and status must not be NULL");
  if (dtype == POGS_AMD_F64) {
    ManyShapes<double> sh;
    sh.set_ragged(k, m, n);
    solve_many_t<double>(ord, sh, A, mem, device, f, g, rho, p, out);
  } else {
    ManyShapes<float> sh;
    sh.set_ragged(k, m, n);
    solve_many_t<float>(ord, sh, A, mem, device, f, g, rho, p, out);
  }
}

void solve_many(int dtype, int ord, int k, size_t m, size_t n, const void *A, int mem, int device, const FnHost *f,
                const FnHost *g, const double *rho, const SolveParams &p, const BatchOut &out) {
  many_check_args(dtype, ord, k, m, n, A, mem);
  POGS_CHECK(out.x && out.final_iter && out.status, "many-problem solve: x, final_iter and status must not be NULL");
  if (dtype == POGS_AMD_F64) {
    ManyShapes<double> sh;
    sh.set_uniform(k, m, n);
    solve_many_t<double>(ord, sh, A, mem, device, f, g, rho, p, out);
  } else {
    ManyShapes<float> sh;
    sh.set_uniform(k, m, n);
    solve_many_t<float>(ord, sh, A, mem, device, f, g, rho, p, out);
  }
}

void many_setup_check(int dtype, int ord, int k, size_t m, size_t n, const void *A, int mem, void *A_eq, void *d,
                      void *e, double *nrmA, void *W) {
  many_check_uniform("many setup check", dtype, ord, k, m, n, A, mem);
  if (dtype == POGS_AMD_F64)
    many_setup_check_t<double>(ord, k, m, n, A, mem, static_cast<double *>(A_eq), static_cast<double *>(d),
                               static_cast<double *>(e), nrmA, static_cast<double *>(W));
  else
    many_setup_check_t<float>(ord, k, m, n, A, mem, static_cast<float *>(A_eq), static_cast<float *>(d),
                              static_cast<float *>(e), nrmA, static_cast<float *>(W));
}

}  // namespace pogs_amd

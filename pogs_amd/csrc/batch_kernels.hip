// Kernels of the batched dense solves: see batch_kernels.h, batch_admm.h (the loop) and dense_batch.h (the passes).
//
// Determinism: every multi-vector product is a v_mfma_*_16x16x4 chain, which is a k-ordered FMA chain per output
// element, so the arithmetic of problem j depends neither on the other vectors nor on j's slot; the partials of
// row blocks / waves are summed in a fixed order, and the row-block partition depends on the matrix shape only.
#include "batch_kernels.h"
#include "reduce.h"
#include "stream.h"
#include "vec_kernels.h"

namespace pogs_amd {
namespace {

template <typename T>
struct BatchMfma;
template <>
struct BatchMfma<float> {
  typedef float acc __attribute__((ext_vector_type(4)));
  static __device__ __forceinline__ acc mfma(float a, float b, acc c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  }
  // row of the 16 x 16 result held in register r of lane l (column l & 15)
  static __device__ __forceinline__ int row(int lane, int r) { return 4 * (lane >> 4) + r; }
};
template <>
struct BatchMfma<double> {
  typedef double acc __attribute__((ext_vector_type(4)));
  static __device__ __forceinline__ acc mfma(double a, double b, acc c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ int row(int lane, int r) { return (lane >> 4) + 4 * r; }
};

// ---- K row dots: Y[p][row] = sum_c M[row][c] X[p][c] over the problems p of the slots -------------------------
// A workgroup (4 waves) takes 64 rows (four 16-row groups); the waves walk the columns in interleaved steps of
// 4 * VEC columns: lane l loads 16 bytes of row (l & 15) at column c0 + VEC (l >> 4) for each row group, and the
// same 16 bytes of vector (l & 15), so element t of the load is MFMA t's k-slice (A[i][k] = M[r0 + i][c0 + VEC k + t],
// B[k][j] = X_j[c0 + VEC k + t]).  One vector load serves four row groups.  The four waves' partial dots are added
// in wave order through LDS.  TRI: the lower (c <= row) or upper (c >= row) triangle of a square factor only --
// entries outside it are not read (and whatever the storage holds there does not matter); columns >= cols are zero.

template <typename T, int TRI>
__global__ void __launch_bounds__(256) batch_rows_kernel(const T *__restrict__ M, size_t ldm, int rows, int cols,
                                                         int cols_pad, const T *__restrict__ X, size_t ldx,
                                                         T *__restrict__ Y, size_t ldy, BatchSlots sl) {
  using V = typename Vec16<T>::type;
  using MF = BatchMfma<T>;
  constexpr int VEC = Vec16<T>::N;
  constexpr int STEP = 4 * VEC;   // columns per wave step
  __shared__ T red[4][kBRowsPerWg][17];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i = lane & 15, q = lane >> 4;
  const int r0 = blockIdx.x * kBRowsPerWg;
  int cbeg = 0, cend = cols;
  if (TRI == kLower) cend = min(cols, r0 + kBRowsPerWg);
  if (TRI == kUpper) cbeg = (r0 / (4 * STEP)) * (4 * STEP);
  const bool vec_on = i < sl.nact;
  const T *xp = X + (vec_on ? static_cast<size_t>(sl.act[i]) * ldx : 0);
  typename MF::acc acc[kBRowGroups];
#pragma unroll
  for (int g = 0; g < kBRowGroups; ++g) acc[g] = typename MF::acc{0, 0, 0, 0};
  for (int c0 = cbeg + w * STEP; c0 < cend; c0 += 4 * STEP) {
    const int c = c0 + VEC * q;
    V xv, av[kBRowGroups];
    T *xe = reinterpret_cast<T *>(&xv);
#pragma unroll
    for (int t = 0; t < VEC; ++t) xe[t] = 0;
    if (vec_on && c < cols_pad) xv = *reinterpret_cast<const V *>(xp + c);
#pragma unroll
    for (int g = 0; g < kBRowGroups; ++g) {
      const int row = r0 + 16 * g + i;
      T *ae = reinterpret_cast<T *>(&av[g]);
#pragma unroll
      for (int t = 0; t < VEC; ++t) ae[t] = 0;
      bool ok = row < rows && c < cols_pad;
      if (TRI == kLower) ok = ok && c <= row;
      if (TRI == kUpper) ok = ok && c + VEC - 1 >= row;
      if (ok) {
        const T *rp = M + static_cast<size_t>(row) * ldm + c;
        av[g] = (TRI == kFull) ? stream_load<V>(rp) : *reinterpret_cast<const V *>(rp);
      }
    }
#pragma unroll
    for (int g = 0; g < kBRowGroups; ++g) {
      const int row = r0 + 16 * g + i;
      T *ae = reinterpret_cast<T *>(&av[g]);
#pragma unroll
      for (int t = 0; t < VEC; ++t) {
        bool keep = c + t < cols;
        if (TRI == kLower) keep = keep && c + t <= row;
        if (TRI == kUpper) keep = keep && c + t >= row;
        acc[g] = MF::mfma(keep ? ae[t] : static_cast<T>(0), xe[t], acc[g]);
      }
    }
  }
#pragma unroll
  for (int g = 0; g < kBRowGroups; ++g)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[w][16 * g + MF::row(lane, r)][i] = acc[g][r];
  __syncthreads();
  for (int o = threadIdx.x; o < kBRowsPerWg * 16; o += 256) {
    const int rr = o >> 4, j = o & 15;
    const int row = r0 + rr;
    if (j < sl.nact && row < rows) {
      const T v = ((red[0][rr][j] + red[1][rr][j]) + red[2][rr][j]) + red[3][rr][j];
      Y[static_cast<size_t>(sl.act[j]) * ldy + row] = v;
    }
  }
}

// ---- K column sums, first stage: part[rb][p][c] = sum over the rows of row block rb of M[row][c] U[p][row] ------
// A workgroup (4 waves) takes a slab of 16 VEC columns and one row block; the waves take interleaved quads of rows.
// Lane l loads 16 bytes of row (4 quad + (l >> 4)) at column cs + VEC (l & 15) and the vector value U_(l & 15) of
// that row, so element t of the load is MFMA t's A (rows of the 16 x 16 result = columns cs + VEC i + t) and the
// vector value its B (k = the row within the quad).  Four quads are loaded per step.
template <typename T>
__global__ void __launch_bounds__(256) batch_cols_kernel(const T *__restrict__ M, size_t ldm, int rows, int cols_pad,
                                                         int rows_per_block, const T *__restrict__ U, size_t ldu,
                                                         T *__restrict__ part, int kb, BatchSlots sl) {
  using V = typename Vec16<T>::type;
  using MF = BatchMfma<T>;
  constexpr int VEC = Vec16<T>::N;
  constexpr int SLAB = 16 * VEC;
  constexpr int QU = 4;   // quads per wave step
  __shared__ T red[4][SLAB][17];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i = lane & 15, k = lane >> 4;
  const int cs = blockIdx.x * SLAB;
  const int rb = blockIdx.y;
  const int rlo = rb * rows_per_block, rhi = min(rows, rlo + rows_per_block);
  const bool vec_on = i < sl.nact;
  const T *up = U + (vec_on ? static_cast<size_t>(sl.act[i]) * ldu : 0);
  const int c = cs + VEC * i;
  typename MF::acc acc[VEC];
#pragma unroll
  for (int t = 0; t < VEC; ++t) acc[t] = typename MF::acc{0, 0, 0, 0};
  for (int rq = rlo + 4 * w; rq < rhi; rq += 16 * QU) {
    V av[QU];
    T uv[QU];
#pragma unroll
    for (int u = 0; u < QU; ++u) {
      const int row = rq + 16 * u + k;
      T *ae = reinterpret_cast<T *>(&av[u]);
#pragma unroll
      for (int t = 0; t < VEC; ++t) ae[t] = 0;
      uv[u] = 0;
      if (row < rhi) {
        if (c < cols_pad) av[u] = stream_load<V>(M + static_cast<size_t>(row) * ldm + c);
        if (vec_on) uv[u] = up[row];
      }
    }
#pragma unroll
    for (int u = 0; u < QU; ++u) {
      const T *ae = reinterpret_cast<const T *>(&av[u]);
#pragma unroll
      for (int t = 0; t < VEC; ++t) acc[t] = MF::mfma(ae[t], uv[u], acc[t]);
    }
  }
#pragma unroll
  for (int t = 0; t < VEC; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[w][VEC * MF::row(lane, r) + t][i] = acc[t][r];
  __syncthreads();
  for (int o = threadIdx.x; o < SLAB * 16; o += 256) {
    const int cc = o >> 4, j = o & 15;
    const int col = cs + cc;
    if (j < sl.nact && col < cols_pad) {
      const T v = ((red[0][cc][j] + red[1][cc][j]) + red[2][cc][j]) + red[3][cc][j];
      part[(static_cast<size_t>(rb) * kb + sl.act[j]) * cols_pad + col] = v;
    }
  }
}

// second stage: Z[p][c] = (sum_rb part[rb][p][c], in row-block order) (+ add[p][c]); columns >= cols are zero
template <typename T>
__global__ void __launch_bounds__(256) batch_cols_reduce_kernel(const T *__restrict__ part, int nrb, int kb, int cols,
                                                                int cols_pad, const T *__restrict__ add, T *__restrict__ Z,
                                                                size_t ldz, BatchSlots sl) {
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= cols_pad) return;
  const int p = sl.act[blockIdx.y];
  T v = 0;
  for (int rb = 0; rb < nrb; ++rb) v += part[(static_cast<size_t>(rb) * kb + p) * cols_pad + col];
  if (add) v = v + add[static_cast<size_t>(p) * ldz + col];
  Z[static_cast<size_t>(p) * ldz + col] = col < cols ? v : static_cast<T>(0);
}

// ---- mixed storage: the two passes over A on a float copy of the matrix, fp64 vectors and arithmetic ---------------
// batch_rows_kernel<double, kFull> and batch_cols_kernel<double> with the matrix operand stored as floats
// (DenseSolver's A32_, stream_mixed.h): 4 instead of 8 bytes per entry, each float widened where it is used (exact).
// Every output element is added up in the fp64 kernel's order -- the same columns in the same (wave, step, MFMA, k)
// places, the same rows in the same (wave, step, quad, k) places -- so the result is, bit for bit, what the fp64
// kernel returns for the widened matrix.  Loads are unconditional on addresses clamped into the matrix, masks are
// applied afterwards (stream_mixed.h: a guarded load is a branch, and behind it every load is waited for on its own).

__device__ __forceinline__ float2 stream_load_f2(const float *p) {
#if POGS_AMD_NT_LOADS
  typedef unsigned int raw8 __attribute__((ext_vector_type(2)));
  const raw8 raw = __builtin_nontemporal_load(reinterpret_cast<const raw8 *>(p));
  float2 out;
  __builtin_memcpy(&out, &raw, 8);
  return out;
#else
  return *reinterpret_cast<const float2 *>(p);
#endif
}

// Row dots.  The fp64 geometry (VEC = 2, STEP = 8) with 8-byte loads: lane l loads the two floats of row (l & 15) at
// column c0 + 2 (l >> 4), which are the two doubles the fp64 kernel's lane loads -- the mapping of columns to
// (wave, step, MFMA, k) needs no further work.  Whatever the float row holds from cols on is masked.
__global__ void __launch_bounds__(256) batch_rows_mixed_kernel(const float *__restrict__ M, size_t ldm, int rows,
                                                               int cols, int cols_pad, const double *__restrict__ X,
                                                               size_t ldx, double *__restrict__ Y, size_t ldy,
                                                               BatchSlots sl) {
  using MF = BatchMfma<double>;
  constexpr int VEC = Vec16<double>::N;
  constexpr int STEP = 4 * VEC;
  __shared__ double red[4][kBRowsPerWg][17];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i = lane & 15, q = lane >> 4;
  const int r0 = blockIdx.x * kBRowsPerWg;
  const bool vec_on = i < sl.nact;
  const double *xp = X + (vec_on ? static_cast<size_t>(sl.act[i]) * ldx : 0);
  const float *rp[kBRowGroups];
  bool row_in[kBRowGroups];
  MF::acc acc[kBRowGroups];
#pragma unroll
  for (int g = 0; g < kBRowGroups; ++g) {
    const int row = r0 + 16 * g + i;
    row_in[g] = row < rows;
    rp[g] = M + static_cast<size_t>(row_in[g] ? row : rows - 1) * ldm;
    acc[g] = MF::acc{0, 0, 0, 0};
  }
  struct Tile {
    float2 a[kBRowGroups];
    double2 x;
  };
  // (unconditional: a lane past the row's end reads column 0 again and is masked in `use`)
  auto load = [&](int cb, Tile &t) {
    const int c = cb + VEC * q;
    const int cc = c < cols_pad ? c : 0;   // (cc + 1 < cols_pad <= min(ldx, ldm))
    t.x = *reinterpret_cast<const double2 *>(xp + cc);
#pragma unroll
    for (int g = 0; g < kBRowGroups; ++g) t.a[g] = stream_load_f2(rp[g] + cc);
  };
  auto use = [&](int cb, const Tile &t) {
    const int c = cb + VEC * q;
    const bool x_on = vec_on && c < cols_pad;
    const double xe[VEC] = {x_on ? t.x.x : 0.0, x_on ? t.x.y : 0.0};
#pragma unroll
    for (int g = 0; g < kBRowGroups; ++g) {
      const float ae[VEC] = {t.a[g].x, t.a[g].y};
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const bool keep = row_in[g] && c + k < cols;
        acc[g] = MF::mfma(keep ? static_cast<double>(ae[k]) : 0.0, xe[k], acc[g]);
      }
    }
  };
  // (the wave index as a scalar: the loop's control is then the scalar unit's)
  for (int cb = __builtin_amdgcn_readfirstlane(w) * STEP; cb < cols; cb += 4 * STEP) {
    Tile t;
    load(cb, t);
    use(cb, t);
  }
#pragma unroll
  for (int g = 0; g < kBRowGroups; ++g)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[w][16 * g + MF::row(lane, r)][i] = acc[g][r];
  __syncthreads();
  for (int o = threadIdx.x; o < kBRowsPerWg * 16; o += 256) {
    const int rr = o >> 4, j = o & 15;
    const int row = r0 + rr;
    if (j < sl.nact && row < rows) {
      const double v = ((red[0][rr][j] + red[1][rr][j]) + red[2][rr][j]) + red[3][rr][j];
      Y[static_cast<size_t>(sl.act[j]) * ldy + row] = v;
    }
  }
}

// Column sums, first stage.  A column's chain runs over rows only, so the slab width is free: 16-byte loads of four
// floats over a slab of 64 columns, four accumulators; rows are dealt as in batch_cols_kernel<double> (wave w takes the
// quads rlo + 4 w + 64 s, four quads per step, k = the row within the quad).  cols_pad = round_up(cols, 2) is the
// length of a partials record; the float row runs to round_up(cols, 4) <= ldm, so the last vector of a row may cover
// two columns with no slot (cols_pad % 4 == 2): they are loaded and summed, and never stored.
__global__ void __launch_bounds__(256) batch_cols_mixed_kernel(const float *__restrict__ M, size_t ldm, int rows,
                                                               int cols_pad, int rows_per_block,
                                                               const double *__restrict__ U, size_t ldu,
                                                               double *__restrict__ part, int kb, BatchSlots sl) {
  using MF = BatchMfma<double>;
  constexpr int VEC = 4;
  constexpr int SLAB = kBatchColsMixedSlab;
  constexpr int QU = 4;
  static_assert(SLAB == 16 * VEC, "slab width");
  __shared__ double red[4][SLAB][17];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i = lane & 15, k = lane >> 4;
  const int cs = blockIdx.x * SLAB;
  const int rb = blockIdx.y;
  const int rlo = rb * rows_per_block, rhi = min(rows, rlo + rows_per_block);
  const bool vec_on = i < sl.nact;
  const double *up = U + (vec_on ? static_cast<size_t>(sl.act[i]) * ldu : 0);
  const int c = cs + VEC * i;
  const bool col_in = c < cols_pad;
  const float *cp = M + (col_in ? c : 0);   // (c + 3 < round_up(cols_pad, 4) <= ldm)
  MF::acc acc[VEC];
#pragma unroll
  for (int t = 0; t < VEC; ++t) acc[t] = MF::acc{0, 0, 0, 0};
  for (int rq = rlo + 4 * w; rq < rhi; rq += 16 * QU) {
    float4 av[QU];
    double uv[QU];
#pragma unroll
    for (int u = 0; u < QU; ++u) {
      const int row = rq + 16 * u + k;
      const int rc = row < rhi ? row : rhi - 1;
      av[u] = stream_load<float4>(cp + static_cast<size_t>(rc) * ldm);
      uv[u] = up[rc];
    }
#pragma unroll
    for (int u = 0; u < QU; ++u) {
      const int row = rq + 16 * u + k;
      const bool a_on = row < rhi && col_in;
      const double ub = (row < rhi && vec_on) ? uv[u] : 0.0;
      const float ae[VEC] = {av[u].x, av[u].y, av[u].z, av[u].w};
#pragma unroll
      for (int t = 0; t < VEC; ++t) acc[t] = MF::mfma(a_on ? static_cast<double>(ae[t]) : 0.0, ub, acc[t]);
    }
  }
#pragma unroll
  for (int t = 0; t < VEC; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[w][VEC * MF::row(lane, r) + t][i] = acc[t][r];
  __syncthreads();
  for (int o = threadIdx.x; o < SLAB * 16; o += 256) {
    const int cc = o >> 4, j = o & 15;
    const int col = cs + cc;
    if (j < sl.nact && col < cols_pad) {
      const double v = ((red[0][cc][j] + red[1][cc][j]) + red[2][cc][j]) + red[3][cc][j];
      part[(static_cast<size_t>(rb) * kb + sl.act[j]) * cols_pad + col] = v;
    }
  }
}

// ---- element-wise stages, blockIdx.y = slot; x blocks first, then y blocks ---------------------------------------
// prox + over-relaxation (pogs.cpp:257-278; admm_pre_kernel), sums {w h, w^2, h^2}
template <typename T>
__global__ void __launch_bounds__(kVecTpb) batch_pre_kernel(BatchVecArgs<T> a) {
  __shared__ double s_red[3 * (kVecTpb / 64)];
  const int p = a.sl.act[blockIdx.y];
  const bool is_x = static_cast<int>(blockIdx.x) < a.bx;
  const int blk = is_x ? blockIdx.x : blockIdx.x - a.bx;
  const int n = is_x ? a.n : a.m;
  const size_t off = static_cast<size_t>(p) * (is_x ? a.ldx : a.ldy);
  const FnView<T> fn = a.fg[2 * p + (is_x ? 1 : 0)];
  const T *cur = (is_x ? a.x_cur : a.y_cur) + off;
  const T *zt = (is_x ? a.xt : a.yt) + off;
  T *z12 = (is_x ? a.x12 : a.y12) + off;
  T *ztemp = (is_x ? a.xtemp : a.ytemp) + off;
  const T rho = a.rho[p], zsc = a.zs[p];
  double acc[3] = {0.0, 0.0, 0.0};
  const int e = blk * kVecTpb + threadIdx.x;
  if (e < n) {
    const T prev = cur[e];
    const T zs = zsc * zt[e];
    const T v = prev - zs;
    const T h = dev::ProxEval(fn.h[e], fn.a[e], fn.b[e], fn.c[e], fn.d[e], fn.e[e], v, rho);
    const T wv = v - h;
    z12[e] = h;
    ztemp[e] = zs + a.alpha * h + (static_cast<T>(1) - a.alpha) * prev;
    dev::prod_acc(acc[0], wv, h);
    dev::prod_acc(acc[1], wv, wv);
    dev::prod_acc(acc[2], h, h);
  }
  dev::block_sum<3, kVecTpb>(acc, s_red);
  if (threadIdx.x == 0) {
    double *out = a.part + (static_cast<size_t>(p) * (a.bx + a.by) + blockIdx.x) * 3;
    out[0] = acc[0]; out[1] = acc[1]; out[2] = acc[2];
  }
}

// projection tail (ProjTailOp): sums {(zprev - znew)^2, (z12 - znew)^2}, ztemp -= znew
template <typename T>
__global__ void __launch_bounds__(kVecTpb) batch_tail_kernel(BatchVecArgs<T> a) {
  __shared__ double s_red[2 * (kVecTpb / 64)];
  const int p = a.sl.act[blockIdx.y];
  const bool is_x = static_cast<int>(blockIdx.x) < a.bx;
  const int blk = is_x ? blockIdx.x : blockIdx.x - a.bx;
  const int n = is_x ? a.n : a.m;
  const size_t off = static_cast<size_t>(p) * (is_x ? a.ldx : a.ldy);
  double acc[2] = {0.0, 0.0};
  const int e = blk * kVecTpb + threadIdx.x;
  if (e < n) {
    const T zn = (is_x ? a.x_new : a.y_new)[off + e];
    const T pv = (is_x ? a.x_cur : a.y_cur)[off + e] - zn;
    const T qv = (is_x ? a.x12 : a.y12)[off + e] - zn;
    dev::prod_acc(acc[0], pv, pv);
    dev::prod_acc(acc[1], qv, qv);
    (is_x ? a.xtemp : a.ytemp)[off + e] -= zn;
  }
  dev::block_sum<2, kVecTpb>(acc, s_red);
  if (threadIdx.x == 0) {
    double *out = a.part + (static_cast<size_t>(p) * (a.bx + a.by) + blockIdx.x) * 2;
    out[0] = acc[0]; out[1] = acc[1];
  }
}

// u = y12 + zs yt - yprev  (the y half of the exact dual residual, pogs.cpp:366-368)
template <typename T>
__global__ void __launch_bounds__(kVecTpb) batch_exact_u_kernel(BatchVecArgs<T> a) {
  const int p = a.sl.act[blockIdx.y];
  const int e = blockIdx.x * kVecTpb + threadIdx.x;
  if (e >= a.m) return;
  const size_t o = static_cast<size_t>(p) * a.ldy + e;
  a.u[o] = a.y12[o] + a.zs[p] * a.yt[o] - a.y_cur[o];
}

// exact residuals (ExactRowOp / ExactColOp): y blocks sum (A x12 - y12)^2, x blocks (A^T u + x12 + zs xt - xprev)^2
template <typename T>
__global__ void __launch_bounds__(kVecTpb) batch_exact_kernel(BatchVecArgs<T> a) {
  __shared__ double s_red[kVecTpb / 64];
  const int p = a.sl.act[blockIdx.y];
  const bool is_x = static_cast<int>(blockIdx.x) < a.bx;
  const int blk = is_x ? blockIdx.x : blockIdx.x - a.bx;
  double acc[1] = {0.0};
  const int e = blk * kVecTpb + threadIdx.x;
  if (is_x && e < a.n) {
    const size_t o = static_cast<size_t>(p) * a.ldx + e;
    const T v = a.zx[o] + a.x12[o] + a.zs[p] * a.xt[o] - a.x_cur[o];
    dev::prod_acc(acc[0], v, v);
  } else if (!is_x && e < a.m) {
    const size_t o = static_cast<size_t>(p) * a.ldy + e;
    const T r = a.zy[o] - a.y12[o];
    dev::prod_acc(acc[0], r, r);
  }
  dev::block_sum<1, kVecTpb>(acc, s_red);
  if (threadIdx.x == 0) a.part[static_cast<size_t>(p) * (a.bx + a.by) + blockIdx.x] = acc[0];
}

// warm begin, before the products: x12 = x0 / e (x blocks), u = l0 / d (y blocks)   (pogs.cpp:146, 152)
template <typename T>
__global__ void __launch_bounds__(kVecTpb) batch_warm_scale_kernel(BatchWarmArgs<T> a) {
  const int p = a.sl.act[blockIdx.y];
  const bool is_x = static_cast<int>(blockIdx.x) < a.bx;
  const int blk = is_x ? blockIdx.x : blockIdx.x - a.bx;
  const int e = blk * kVecTpb + threadIdx.x;
  if (is_x && e < a.n) {
    const size_t o = static_cast<size_t>(p) * a.ldx + e;
    a.x12[o] = a.x0[o] / a.e[e];
  } else if (!is_x && e < a.m) {
    const size_t o = static_cast<size_t>(p) * a.ldy + e;
    a.u[o] = a.l0[o] / a.d[e];
  }
}

// warm begin, after the products: x = x0 / e, xt = (A^T t) (1 / rho) (x blocks); y = A x, yt = t (-1 / rho) (y blocks)
template <typename T>
__global__ void __launch_bounds__(kVecTpb) batch_warm_close_kernel(BatchWarmArgs<T> a) {
  const int p = a.sl.act[blockIdx.y];
  const bool is_x = static_cast<int>(blockIdx.x) < a.bx;
  const int blk = is_x ? blockIdx.x : blockIdx.x - a.bx;
  const int e = blk * kVecTpb + threadIdx.x;
  if (is_x && e < a.n) {
    const size_t o = static_cast<size_t>(p) * a.ldx + e;
    a.x_cur[o] = a.x12[o];
    a.xt[o] = a.zx[o] * a.pos[p];
  } else if (!is_x && e < a.m) {
    const size_t o = static_cast<size_t>(p) * a.ldy + e;
    a.y_cur[o] = a.zy[o];
    a.yt[o] = a.u[o] * a.neg[p];
  }
}

__global__ void __launch_bounds__(256) batch_sum_kernel(BatchSumJobs jobs, BatchSlots sl, double *out) {
  __shared__ double s_red[3 * 4];
  const BatchSumJob jb = jobs.j[blockIdx.x];
  const int p = sl.act[blockIdx.y];
  double acc[3] = {0.0, 0.0, 0.0};
  const double *src = jb.part + static_cast<size_t>(p) * jb.nblk * jb.ns;
  for (int b = jb.b0 + static_cast<int>(threadIdx.x); b < jb.b1; b += 256)
#pragma unroll
    for (int q = 0; q < 3; ++q)
      if (q < jb.ns) acc[q] += src[static_cast<size_t>(b) * jb.ns + q];
  dev::block_sum<3, 256>(acc, s_red);
  if (threadIdx.x == 0)
#pragma unroll
    for (int q = 0; q < 3; ++q)
      if (q < jb.ns) out[static_cast<size_t>(p) * kBatchRec + jb.slot + q] = acc[q];
}


}  // namespace

template <typename T>
void launch_batch_rows(int tri, const T *M, size_t ldm, int rows, int cols, int cols_pad, const T *X, size_t ldx, T *Y,
                       size_t ldy, const BatchSlots &sl, hipStream_t s) {
  const dim3 grid((rows + kBRowsPerWg - 1) / kBRowsPerWg);
  if (tri == kLower) hipLaunchKernelGGL((batch_rows_kernel<T, kLower>), grid, dim3(256), 0, s, M, ldm, rows, cols, cols_pad, X, ldx, Y, ldy, sl);
  else if (tri == kUpper) hipLaunchKernelGGL((batch_rows_kernel<T, kUpper>), grid, dim3(256), 0, s, M, ldm, rows, cols, cols_pad, X, ldx, Y, ldy, sl);
  else hipLaunchKernelGGL((batch_rows_kernel<T, kFull>), grid, dim3(256), 0, s, M, ldm, rows, cols, cols_pad, X, ldx, Y, ldy, sl);
}

template <typename T>
void launch_batch_cols(const T *M, size_t ldm, int rows, int cols_pad, int rows_per_block, int nrb, const T *U,
                       size_t ldu, T *part, int kb, const BatchSlots &sl, hipStream_t s) {
  constexpr int SLAB = 16 * Vec16<T>::N;
  static_assert(SLAB == batch_cols_slab<T>(), "slab width");
  hipLaunchKernelGGL(batch_cols_kernel<T>, dim3((cols_pad + SLAB - 1) / SLAB, nrb), dim3(256), 0, s, M, ldm, rows,
                     cols_pad, rows_per_block, U, ldu, part, kb, sl);
}

template <typename T>
void launch_batch_cols_reduce(const T *part, int nrb, int kb, int cols, int cols_pad, const T *add, T *Z, size_t ldz,
                              const BatchSlots &sl, hipStream_t s) {
  hipLaunchKernelGGL(batch_cols_reduce_kernel<T>, dim3((cols_pad + 255) / 256, sl.nact), dim3(256), 0, s, part, nrb, kb,
                     cols, cols_pad, add, Z, ldz, sl);
}

void launch_batch_rows_mixed(const float *M, size_t ldm, int rows, int cols, int cols_pad, const double *X, size_t ldx,
                             double *Y, size_t ldy, const BatchSlots &sl, hipStream_t s) {
  hipLaunchKernelGGL(batch_rows_mixed_kernel, dim3((rows + kBRowsPerWg - 1) / kBRowsPerWg), dim3(256), 0, s, M, ldm,
                     rows, cols, cols_pad, X, ldx, Y, ldy, sl);
}

void launch_batch_cols_mixed(const float *M, size_t ldm, int rows, int cols_pad, int rows_per_block, int nrb,
                             const double *U, size_t ldu, double *part, int kb, const BatchSlots &sl, hipStream_t s) {
  hipLaunchKernelGGL(batch_cols_mixed_kernel, dim3((cols_pad + kBatchColsMixedSlab - 1) / kBatchColsMixedSlab, nrb),
                     dim3(256), 0, s, M, ldm, rows, cols_pad, rows_per_block, U, ldu, part, kb, sl);
}

template <typename T>
void launch_batch_pre(const BatchVecArgs<T> &a, hipStream_t s) {
  hipLaunchKernelGGL(batch_pre_kernel<T>, dim3(a.bx + a.by, a.sl.nact), dim3(kVecTpb), 0, s, a);
}
template <typename T>
void launch_batch_tail(const BatchVecArgs<T> &a, hipStream_t s) {
  hipLaunchKernelGGL(batch_tail_kernel<T>, dim3(a.bx + a.by, a.sl.nact), dim3(kVecTpb), 0, s, a);
}
template <typename T>
void launch_batch_exact_u(const BatchVecArgs<T> &a, hipStream_t s) {
  hipLaunchKernelGGL(batch_exact_u_kernel<T>, dim3(a.by, a.sl.nact), dim3(kVecTpb), 0, s, a);
}
template <typename T>
void launch_batch_exact(const BatchVecArgs<T> &a, hipStream_t s) {
  hipLaunchKernelGGL(batch_exact_kernel<T>, dim3(a.bx + a.by, a.sl.nact), dim3(kVecTpb), 0, s, a);
}
void launch_batch_sums(const BatchSumJobs &jobs, int njobs, const BatchSlots &sl, double *out, hipStream_t s) {
  hipLaunchKernelGGL(batch_sum_kernel, dim3(njobs, sl.nact), dim3(256), 0, s, jobs, sl, out);
}
template <typename T>
void launch_batch_warm_scale(const BatchWarmArgs<T> &a, hipStream_t s) {
  hipLaunchKernelGGL(batch_warm_scale_kernel<T>, dim3(a.bx + a.by, a.sl.nact), dim3(kVecTpb), 0, s, a);
}
template <typename T>
void launch_batch_warm_close(const BatchWarmArgs<T> &a, hipStream_t s) {
  hipLaunchKernelGGL(batch_warm_close_kernel<T>, dim3(a.bx + a.by, a.sl.nact), dim3(kVecTpb), 0, s, a);
}

template <typename T>
void batch_rows_check(int tri, int rows, int cols, const T *M, size_t ldm, int k, const int *act, int nact, const T *X,
                      size_t ldx, T *Y, size_t ldy) {
  constexpr size_t VEC = Vec16<T>::N;
  const BatchSlots sl = checked_batch_slots(k, act, nact);
  POGS_CHECK(tri == kFull || tri == kLower || tri == kUpper, "unknown tri (0 full, 1 lower, 2 upper)");
  POGS_CHECK(rows >= 1 && cols >= 1, "rows and cols must be >= 1");
  POGS_CHECK(tri == kFull || rows == cols, "a triangle needs rows == cols");
  POGS_CHECK(M && X && Y, "null argument");
  const size_t cols_pad = round_up(static_cast<size_t>(cols), VEC);
  POGS_CHECK(ldm >= cols_pad && ldm % VEC == 0, "ldm must be a multiple of VEC and >= round_up(cols, VEC)");
  POGS_CHECK(ldx >= cols_pad && ldx % VEC == 0, "ldx must be a multiple of VEC and >= round_up(cols, VEC)");
  POGS_CHECK(ldy >= static_cast<size_t>(rows), "ldy must be >= rows");
  const size_t nm = static_cast<size_t>(rows) * ldm, nx = static_cast<size_t>(k) * ldx, ny = static_cast<size_t>(k) * ldy;
  DevBuf<T> dM(nm), dX(nx), dY(ny);
  POGS_HIP_CHECK(hipMemcpy(dM.p, M, nm * sizeof(T), hipMemcpyHostToDevice));
  POGS_HIP_CHECK(hipMemcpy(dX.p, X, nx * sizeof(T), hipMemcpyHostToDevice));
  POGS_HIP_CHECK(hipMemcpy(dY.p, Y, ny * sizeof(T), hipMemcpyHostToDevice));
  launch_batch_rows<T>(tri, dM.p, ldm, rows, cols, static_cast<int>(cols_pad), dX.p, ldx, dY.p, ldy, sl, nullptr);
  POGS_HIP_CHECK(hipGetLastError());
  POGS_HIP_CHECK(hipMemcpy(Y, dY.p, ny * sizeof(T), hipMemcpyDeviceToHost));
  POGS_HIP_CHECK(hipDeviceSynchronize());
}

template <typename T>
void batch_cols_check(int rows, int cols, const T *M, size_t ldm, int k, const int *act, int nact, const T *U,
                      size_t ldu, const T *add, T *Z, size_t ldz, int *nrb_used, int *rpb) {
  constexpr size_t VEC = Vec16<T>::N;
  const BatchSlots sl = checked_batch_slots(k, act, nact);
  POGS_CHECK(rows >= 1 && cols >= 1, "rows and cols must be >= 1");
  POGS_CHECK(M && U && Z && nrb_used && rpb, "null argument");
  const size_t cols_pad = round_up(static_cast<size_t>(cols), VEC);
  POGS_CHECK(ldm >= cols_pad && ldm % VEC == 0, "ldm must be a multiple of VEC and >= round_up(cols, VEC)");
  POGS_CHECK(ldu >= static_cast<size_t>(rows), "ldu must be >= rows");
  POGS_CHECK(ldz >= cols_pad, "ldz must be >= round_up(cols, VEC)");
  int rb = 0, nrb = 0;
  batch_cols_partition<T>(rows, static_cast<int>(cols_pad), rb, nrb);
  const size_t nm = static_cast<size_t>(rows) * ldm, nu = static_cast<size_t>(k) * ldu, nz = static_cast<size_t>(k) * ldz;
  DevBuf<T> dM(nm), dU(nu), dZ(nz), dA(add ? nz : 0), part(static_cast<size_t>(nrb) * k * cols_pad);
  POGS_HIP_CHECK(hipMemcpy(dM.p, M, nm * sizeof(T), hipMemcpyHostToDevice));
  POGS_HIP_CHECK(hipMemcpy(dU.p, U, nu * sizeof(T), hipMemcpyHostToDevice));
  POGS_HIP_CHECK(hipMemcpy(dZ.p, Z, nz * sizeof(T), hipMemcpyHostToDevice));
  if (add) POGS_HIP_CHECK(hipMemcpy(dA.p, add, nz * sizeof(T), hipMemcpyHostToDevice));
  launch_batch_cols<T>(dM.p, ldm, rows, static_cast<int>(cols_pad), rb, nrb, dU.p, ldu, part.p, k, sl, nullptr);
  launch_batch_cols_reduce<T>(part.p, nrb, k, cols, static_cast<int>(cols_pad), add ? dA.p : nullptr, dZ.p, ldz, sl,
                              nullptr);
  POGS_HIP_CHECK(hipGetLastError());
  POGS_HIP_CHECK(hipMemcpy(Z, dZ.p, nz * sizeof(T), hipMemcpyDeviceToHost));
  POGS_HIP_CHECK(hipDeviceSynchronize());
  *nrb_used = nrb;
  *rpb = rb;
}

void batch_rows_mixed_check(int rows, int cols, const float *M, size_t ldm, int k, const int *act, int nact,
                            const double *X, size_t ldx, double *Y, size_t ldy) {
  const BatchSlots sl = checked_batch_slots(k, act, nact);
  POGS_CHECK(rows >= 1 && cols >= 1, "rows and cols must be >= 1");
  POGS_CHECK(M && X && Y, "null argument");
  const size_t cols_pad = round_up(static_cast<size_t>(cols), 2);
  POGS_CHECK(ldm >= round_up(static_cast<size_t>(cols), 4) && ldm % 4 == 0,
             "ldm must be a multiple of 4 and >= round_up(cols, 4)");
  POGS_CHECK(ldx >= cols_pad && ldx % 2 == 0, "ldx must be a multiple of 2 and >= round_up(cols, 2)");
  POGS_CHECK(ldy >= static_cast<size_t>(rows), "ldy must be >= rows");
  const size_t nm = static_cast<size_t>(rows) * ldm, nx = static_cast<size_t>(k) * ldx;
  const size_t ny = static_cast<size_t>(k) * ldy;
  DevBuf<float> dM(nm);
  DevBuf<double> dX(nx), dY(ny);
  POGS_HIP_CHECK(hipMemcpy(dM.p, M, nm * sizeof(float), hipMemcpyHostToDevice));
  POGS_HIP_CHECK(hipMemcpy(dX.p, X, nx * sizeof(double), hipMemcpyHostToDevice));
  POGS_HIP_CHECK(hipMemcpy(dY.p, Y, ny * sizeof(double), hipMemcpyHostToDevice));
  launch_batch_rows_mixed(dM.p, ldm, rows, cols, static_cast<int>(cols_pad), dX.p, ldx, dY.p, ldy, sl, nullptr);
  POGS_HIP_CHECK(hipGetLastError());
  POGS_HIP_CHECK(hipMemcpy(Y, dY.p, ny * sizeof(double), hipMemcpyDeviceToHost));
  POGS_HIP_CHECK(hipDeviceSynchronize());
}

void batch_cols_mixed_check(int rows, int cols, const float *M, size_t ldm, int k, const int *act, int nact,
                            const double *U, size_t ldu, const double *add, double *Z, size_t ldz, int *nrb_used,
                            int *rpb) {
  const BatchSlots sl = checked_batch_slots(k, act, nact);
  POGS_CHECK(rows >= 1 && cols >= 1, "rows and cols must be >= 1");
  POGS_CHECK(M && U && Z && nrb_used && rpb, "null argument");
  const size_t cols_pad = round_up(static_cast<size_t>(cols), 2);
  POGS_CHECK(ldm >= round_up(static_cast<size_t>(cols), 4) && ldm % 4 == 0,
             "ldm must be a multiple of 4 and >= round_up(cols, 4)");
  POGS_CHECK(ldu >= static_cast<size_t>(rows), "ldu must be >= rows");
  POGS_CHECK(ldz >= cols_pad && ldz % 2 == 0, "ldz must be a multiple of 2 and >= round_up(cols, 2)");
  int rb = 0, nrb = 0;
  batch_cols_partition<double>(rows, static_cast<int>(cols_pad), rb, nrb);
  const size_t nm = static_cast<size_t>(rows) * ldm, nu = static_cast<size_t>(k) * ldu;
  const size_t nz = static_cast<size_t>(k) * ldz;
  DevBuf<float> dM(nm);
  DevBuf<double> dU(nu), dZ(nz), dA(add ? nz : 0), part(static_cast<size_t>(nrb) * k * cols_pad);
  POGS_HIP_CHECK(hipMemcpy(dM.p, M, nm * sizeof(float), hipMemcpyHostToDevice));
  POGS_HIP_CHECK(hipMemcpy(dU.p, U, nu * sizeof(double), hipMemcpyHostToDevice));
  POGS_HIP_CHECK(hipMemcpy(dZ.p, Z, nz * sizeof(double), hipMemcpyHostToDevice));
  if (add) POGS_HIP_CHECK(hipMemcpy(dA.p, add, nz * sizeof(double), hipMemcpyHostToDevice));
  launch_batch_cols_mixed(dM.p, ldm, rows, static_cast<int>(cols_pad), rb, nrb, dU.p, ldu, part.p, k, sl, nullptr);
  launch_batch_cols_reduce<double>(part.p, nrb, k, cols, static_cast<int>(cols_pad), add ? dA.p : nullptr, dZ.p, ldz,
                                   sl, nullptr);
  POGS_HIP_CHECK(hipGetLastError());
  POGS_HIP_CHECK(hipMemcpy(Z, dZ.p, nz * sizeof(double), hipMemcpyDeviceToHost));
  POGS_HIP_CHECK(hipDeviceSynchronize());
  *nrb_used = nrb;
  *rpb = rb;
}

#define POGS_BATCH_INST(T)                                                                                             \
  template void launch_batch_rows<T>(int, const T *, size_t, int, int, int, const T *, size_t, T *, size_t,             \
                                     const BatchSlots &, hipStream_t);                                                   \
  template void launch_batch_cols<T>(const T *, size_t, int, int, int, int, const T *, size_t, T *, int,                \
                                     const BatchSlots &, hipStream_t);                                                   \
  template void launch_batch_cols_reduce<T>(const T *, int, int, int, int, const T *, T *, size_t, const BatchSlots &,  \
                                            hipStream_t);                                                                \
  template void launch_batch_pre<T>(const BatchVecArgs<T> &, hipStream_t);                                             \
  template void launch_batch_tail<T>(const BatchVecArgs<T> &, hipStream_t);                                            \
  template void launch_batch_exact_u<T>(const BatchVecArgs<T> &, hipStream_t);                                         \
  template void launch_batch_exact<T>(const BatchVecArgs<T> &, hipStream_t);                                          \
  template void launch_batch_warm_scale<T>(const BatchWarmArgs<T> &, hipStream_t);                                    \
  template void launch_batch_warm_close<T>(const BatchWarmArgs<T> &, hipStream_t);                                    \
  template void batch_rows_check<T>(int, int, int, const T *, size_t, int, const int *, int, const T *, size_t, T *,  \
                                    size_t);                                                                           \
  template void batch_cols_check<T>(int, int, const T *, size_t, int, const int *, int, const T *, size_t, const T *, \
                                    T *, size_t, int *, int *);
POGS_BATCH_INST(float)
POGS_BATCH_INST(double)

}  // namespace pogs_amd

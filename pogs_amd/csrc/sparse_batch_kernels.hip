// Kernels of the batched sparse solves: see sparse_batch_kernels.h and sparse_batch.h (the loop: batch_admm.h).
//
// Multi-vector CSR product.  A row is owned by L lanes of one wave (L = 16 / 32 / 64 from the matrix's mean row
// length, about four non-zeros per lane); lane i takes the row's non-zeros i, i + L, i + 2L, ... in order, reads each stored value and index once and
// gathers the K operand values of that column as one contiguous load from the interleaved copy Xp[col][Kp], feeding
// K fused multiply-adds.  The L partial dots of a row are combined by the xor butterfly over distances L/2, ..., 1.
// With K > 1 its first log2(Kp) stages run as a reduce-scatter (each lane keeps half of its slots and sends the other
// half), which is the same pairing and so the same sums: a + b == b + a in IEEE arithmetic.  So a problem's result
// depends on the matrix alone -- not on K, not on its slot, not on the other vectors.  No atomics; the scalar records
// are summed per workgroup over its row groups in a fixed order.
#include "reduce.h"
#include "sparse_batch_kernels.h"
#include "vec_kernels.h"

namespace pogs_amd {
namespace {

constexpr int kSbTpb = 256;
constexpr int kSbMaxGroups = 4 * (64 >> 4);   // row groups per workgroup at 16 lanes per row
constexpr int kSbMaxRpw = 2048;              // rows per workgroup (their pointers are staged in LDS)

template <int KP>
constexpr int log2_kp() { return KP == 1 ? 0 : KP == 2 ? 1 : KP == 4 ? 2 : KP == 8 ? 3 : 4; }

// xv = Xp[0 .. KP): one contiguous gather (16-byte loads where the slot row is that wide)
template <typename T, int KP>
__device__ __forceinline__ void gather_row(const T *__restrict__ xp, T (&xv)[KP]) {
  constexpr int B = KP * static_cast<int>(sizeof(T));
  if constexpr (B >= 16) {
    using V = typename Vec16<T>::type;
    constexpr int E = Vec16<T>::N;
#pragma unroll
    for (int v = 0; v < B / 16; ++v) {
      const V t = reinterpret_cast<const V *>(xp)[v];
      const T *te = reinterpret_cast<const T *>(&t);
#pragma unroll
      for (int q = 0; q < E; ++q) xv[v * E + q] = te[q];
    }
  } else if constexpr (B == 8 && KP == 2) {
    const float2 t = *reinterpret_cast<const float2 *>(xp);
    xv[0] = t.x;
    xv[1] = t.y;
  } else {
    xv[0] = xp[0];
  }
}

// the non-zeros k = k0, k0 + L, ..., k0 + (U - 1) L of a row ending at e: value and index (zero past the row's end)
template <typename T, int U>
__device__ __forceinline__ void load_chunk(const T *__restrict__ val, const int *__restrict__ ind, int k0, int e, int L,
                                           T (&v)[U], int (&c)[U]) {
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int k = k0 + u * L;
    const bool ok = k < e;
    v[u] = ok ? val[k] : static_cast<T>(0);
    c[u] = ok ? ind[k] : 0;
  }
}

// acc[s] += v[u] Xp[c[u]][s] for the non-zeros of the chunk that lie in the row, in k order
template <typename T, int KP, int U>
__device__ __forceinline__ void fma_chunk(const T *__restrict__ Xp, const T (&v)[U], const int (&c)[U], int k0, int e,
                                          int L, T (&acc)[KP]) {
  T xv[U][KP];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if (k0 + u * L < e) gather_row<T, KP>(Xp + static_cast<size_t>(c[u]) * KP, xv[u]);
  }
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (k0 + u * L < e)
#pragma unroll
      for (int s = 0; s < KP; ++s) acc[s] = dev::fma_(v[u], xv[u][s], acc[s]);
}

// The row pointers of the workgroup's rows are staged in LDS, and the first chunk of a group's next row is loaded
// before the current row's gathers are consumed, so a wave keeps two rows' loads in flight.
template <typename T, int KP>
__global__ void __launch_bounds__(kSbTpb) sp_batch_spmv_kernel(SpBatchCsr<T> M, const T *__restrict__ Xp,
                                                               BatchSlots sl, T *__restrict__ Y, size_t ldy,
                                                               const T *__restrict__ yin, size_t ldin, T beta,
                                                               double *__restrict__ part) {
  constexpr int LK = log2_kp<KP>();
  constexpr int U = (KP * sizeof(T) <= 16) ? 4 : (KP * sizeof(T) <= 32 ? 2 : 1);   // non-zeros in flight per lane
  __shared__ double s_nrm[kSbMaxGroups][kBatchMax];
  __shared__ int s_ptr[kSbMaxRpw + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int L = 1 << M.lshift, gpw = 64 >> M.lshift, G = 4 * gpw;
  const int i = lane & (L - 1);
  const int g = wave * gpw + (lane >> M.lshift);
  const int r0 = blockIdx.x * M.rpw, r1 = min(M.nrows, r0 + M.rpw);
  for (int q = threadIdx.x; q <= r1 - r0; q += kSbTpb) s_ptr[q] = M.ptr[r0 + q];
  __syncthreads();
  // after the reduce-scatter stages lane i holds slot i / (L / KP); the first lane of each such span writes it
  const int myslot = i >> (M.lshift - LK);
  const bool fin = (i & ((L >> LK) - 1)) == 0 && myslot < sl.nact;
  const size_t prob = fin ? static_cast<size_t>(sl.act[myslot]) : 0;
  double nrm = 0.0;
  int a = 0, e = 0;
  if (r0 + g < r1) { a = s_ptr[g]; e = s_ptr[g + 1]; }
  T v[U];
  int c[U];
  load_chunk<T, U>(M.val, M.ind, a + i, e, L, v, c);
  for (int base = r0; base < r1; base += G) {   // (uniform over the workgroup: every lane reaches the shuffles)
    const int r = base + g;
    int an = 0, en = 0;
    if (r + G < r1) { an = s_ptr[r + G - r0]; en = s_ptr[r + G - r0 + 1]; }
    T acc[KP];
#pragma unroll
    for (int s = 0; s < KP; ++s) acc[s] = 0;
    T vn[U];
    int cn[U];
    {
      T xv[U][KP];
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (a + i + u * L < e) gather_row<T, KP>(Xp + static_cast<size_t>(c[u]) * KP, xv[u]);
      load_chunk<T, U>(M.val, M.ind, an + i, en, L, vn, cn);   // the next row's first chunk, in flight meanwhile
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (a + i + u * L < e)
#pragma unroll
          for (int s = 0; s < KP; ++s) acc[s] = dev::fma_(v[u], xv[u][s], acc[s]);
    }
    for (int k = a + i + U * L; k < e; k += U * L) {   // rows longer than one chunk
      load_chunk<T, U>(M.val, M.ind, k, e, L, v, c);
      fma_chunk<T, KP, U>(Xp, v, c, k, e, L, acc);
    }
    // butterfly over distances L/2 .. 1; the first LK stages as a reduce-scatter (L >= 16 >= KP)
    int d = L >> 1;
#pragma unroll
    for (int cc = KP; cc > 1; cc >>= 1) {
      const int h2 = cc >> 1;
      const bool up = (i & d) != 0;
#pragma unroll
      for (int h = 0; h < h2; ++h) {
        const T send = up ? acc[h] : acc[h + h2];
        const T keep = up ? acc[h + h2] : acc[h];
        acc[h] = keep + __shfl_xor(send, d, 64);
      }
      d >>= 1;
    }
    for (; d > 0; d >>= 1) acc[0] = acc[0] + __shfl_xor(acc[0], d, 64);
    if (fin && r < r1) {
      T out = acc[0];
      if (yin) out += beta * yin[prob * ldin + r];
      Y[prob * ldy + r] = out;
      dev::prod_acc(nrm, out, out);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) { v[u] = vn[u]; c[u] = cn[u]; }
    a = an;
    e = en;
  }
  if (part) {
    if (fin) s_nrm[g][myslot] = nrm;
    __syncthreads();
    if (static_cast<int>(threadIdx.x) < sl.nact) {
      double t = 0.0;
      for (int q = 0; q < G; ++q) t += s_nrm[q][threadIdx.x];
      part[static_cast<size_t>(sl.act[threadIdx.x]) * M.grid + blockIdx.x] = t;
    }
  }
}

template <typename T>
__global__ void __launch_bounds__(256) sp_batch_pack_kernel(const T *__restrict__ X, size_t ldx, int n, int lkp,
                                                            BatchSlots sl, T *__restrict__ Xp) {
  const size_t idx = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
  const size_t c = idx >> lkp;
  const int s = static_cast<int>(idx & ((1u << lkp) - 1));
  if (c >= static_cast<size_t>(n)) return;
  Xp[idx] = s < sl.nact ? X[static_cast<size_t>(sl.act[s]) * ldx + c] : static_cast<T>(0);
}

// ---- batched CGLS vector stages, blockIdx.y = slot ---------------------------------------------------------------
// x = xw - x0 (x blocks); r = y0 - yw (y blocks)   (projector_cgls.cpp:62, cgls.h:226-233 with A x_warm = yw)
template <typename T>
__global__ void __launch_bounds__(kVecTpb) sp_batch_cg_init_kernel(SpBatchCgArgs<T> a) {
  const size_t p = static_cast<size_t>(a.sl.act[blockIdx.y]);
  if (static_cast<int>(blockIdx.x) < a.bx) {
    const int e = blockIdx.x * kVecTpb + threadIdx.x;
    if (e < a.n) { const size_t o = p * a.ldx + e; a.x[o] = a.xw[o] - a.x0[o]; }
  } else {
    const int e = (blockIdx.x - a.bx) * kVecTpb + threadIdx.x;
    if (e < a.m) { const size_t o = p * a.ldy + e; a.r[o] = a.y0[o] - a.yw[o]; }
  }
}

// x += alpha p; r -= alpha q; records of |x|^2 (cg_update_xr_kernel)
template <typename T>
__global__ void __launch_bounds__(kVecTpb) sp_batch_cg_xr_kernel(SpBatchCgArgs<T> a) {
  __shared__ double s_red[kVecTpb / 64];
  const size_t p = static_cast<size_t>(a.sl.act[blockIdx.y]);
  const double *cg = a.cg + p * kSbCg;
  const T alpha = static_cast<T>(cg[kSbAlpha]);
  const T neg_alpha = static_cast<T>(-cg[kSbAlpha]);
  if (static_cast<int>(blockIdx.x) >= a.bx) {
    const int e = (blockIdx.x - a.bx) * kVecTpb + threadIdx.x;
    if (e < a.m) { const size_t o = p * a.ldy + e; a.r[o] += neg_alpha * a.q[o]; }
    return;   // (uniform per workgroup)
  }
  double acc[1] = {0.0};
  const int e = blockIdx.x * kVecTpb + threadIdx.x;
  if (e < a.n) {
    const size_t o = p * a.ldx + e;
    const T v = a.x[o] + alpha * a.p[o];
    a.x[o] = v;
    acc[0] = static_cast<double>(v) * v;
  }
  dev::block_sum<1, kVecTpb>(acc, s_red);
  if (threadIdx.x == 0) a.part[p * a.bx + blockIdx.x] = acc[0];
}

// p = s + beta p (p = s on the first); records of |p|^2 (cg_update_p_kernel)
template <typename T>
__global__ void __launch_bounds__(kVecTpb) sp_batch_cg_p_kernel(SpBatchCgArgs<T> a) {
  __shared__ double s_red[kVecTpb / 64];
  const size_t p = static_cast<size_t>(a.sl.act[blockIdx.y]);
  const T beta = a.first ? static_cast<T>(0) : static_cast<T>(a.cg[p * kSbCg + kSbBeta]);
  double acc[1] = {0.0};
  const int e = blockIdx.x * kVecTpb + threadIdx.x;
  if (e < a.n) {
    const size_t o = p * a.ldx + e;
    const T v = a.first ? a.sv[o] : a.sv[o] + beta * a.p[o];
    a.p[o] = v;
    acc[0] = static_cast<double>(v) * v;
  }
  dev::block_sum<1, kVecTpb>(acc, s_red);
  if (threadIdx.x == 0) a.part[p * a.bx + blockIdx.x] = acc[0];
}

// x += x0   (projector_cgls.cpp:75)
template <typename T>
__global__ void __launch_bounds__(kVecTpb) sp_batch_cg_close_kernel(SpBatchCgArgs<T> a) {
  const size_t p = static_cast<size_t>(a.sl.act[blockIdx.y]);
  const int e = blockIdx.x * kVecTpb + threadIdx.x;
  if (e < a.n) { const size_t o = p * a.ldx + e; a.x[o] = a.x0[o] + a.x[o]; }
}

// cg_alpha_kernel / cg_beta_kernel / set_gamma_kernel, one thread per slot
__global__ void sp_batch_cg_scalars_kernel(int mode, BatchSlots sl, const double *sums, double *cg, double shift,
                                           double eps) {
  const int t = threadIdx.x;
  if (t >= sl.nact) return;
  const size_t p = static_cast<size_t>(sl.act[t]);
  const double *S = sums + p * kBatchRec;
  double *c = cg + p * kSbCg;
  if (mode == 0) {
    c[kSbGamma] = S[kSbS2];
    c[kSbIndef] = 0.0;
  } else if (mode == 1) {
    double delta = S[kSbQ2] + shift * S[kSbP2];
    if (delta <= 0.0) c[kSbIndef] = 1.0;
    if (delta == 0.0) delta = eps;
    c[kSbDelta] = delta;
    c[kSbAlpha] = c[kSbGamma] / delta;
  } else {
    const double g1 = c[kSbGamma], g = S[kSbS2];
    c[kSbGamma] = g;
    c[kSbBeta] = g / g1;
  }
}

}  // namespace

template <typename T>
static SpBatchCsr<T> geometry(const T *val, const int *ind, const int *ptr, int nrows, size_t nnz, int num_cu) {
  SpBatchCsr<T> M;
  M.val = val; M.ind = ind; M.ptr = ptr; M.nrows = nrows;
  const double mean = nrows > 0 ? static_cast<double>(nnz) / nrows : 0.0;
  M.lshift = 4;   // 16 lanes per row at least: the reduce-scatter needs L >= 16 >= Kp
  while (M.lshift < 6 && 4.0 * (1 << M.lshift) < mean) ++M.lshift;   // up to ~4 non-zeros per lane
  const int G = 4 * (64 >> M.lshift);
  const long long target = 16LL * std::max(1, num_cu);   // workgroups
  M.rpw = std::min(G * std::max(1, ceil_div(nrows, static_cast<long long>(G) * target)), kSbMaxRpw);
  M.grid = std::max(1, ceil_div(nrows, M.rpw));
  return M;
}
SpBatchCsr<float> sp_batch_geometry(const float *val, const int *ind, const int *ptr, int nrows, size_t nnz, int num_cu) {
  return geometry(val, ind, ptr, nrows, nnz, num_cu);
}
SpBatchCsr<double> sp_batch_geometry(const double *val, const int *ind, const int *ptr, int nrows, size_t nnz,
                                     int num_cu) {
  return geometry(val, ind, ptr, nrows, nnz, num_cu);
}

template <typename T>
void launch_sp_batch_pack(const T *X, size_t ldx, int n, const BatchSlots &sl, T *Xp, hipStream_t s) {
  const int kp = sp_batch_kp(sl.nact);
  int lkp = 0;
  while ((1 << lkp) < kp) ++lkp;
  const size_t tot = static_cast<size_t>(n) * kp;
  hipLaunchKernelGGL(sp_batch_pack_kernel<T>, dim3(static_cast<unsigned>((tot + 255) / 256)), dim3(256), 0, s, X, ldx,
                     n, lkp, sl, Xp);
}

template <typename T>
void launch_sp_batch_spmv(const SpBatchCsr<T> &M, const T *Xp, const BatchSlots &sl, T *Y, size_t ldy, const T *yin,
                          size_t ldin, T beta, double *part, hipStream_t s) {
  const dim3 grid(M.grid), block(kSbTpb);
  switch (sp_batch_kp(sl.nact)) {
    case 1: hipLaunchKernelGGL((sp_batch_spmv_kernel<T, 1>), grid, block, 0, s, M, Xp, sl, Y, ldy, yin, ldin, beta, part); break;
    case 2: hipLaunchKernelGGL((sp_batch_spmv_kernel<T, 2>), grid, block, 0, s, M, Xp, sl, Y, ldy, yin, ldin, beta, part); break;
    case 4: hipLaunchKernelGGL((sp_batch_spmv_kernel<T, 4>), grid, block, 0, s, M, Xp, sl, Y, ldy, yin, ldin, beta, part); break;
    case 8: hipLaunchKernelGGL((sp_batch_spmv_kernel<T, 8>), grid, block, 0, s, M, Xp, sl, Y, ldy, yin, ldin, beta, part); break;
    default: hipLaunchKernelGGL((sp_batch_spmv_kernel<T, 16>), grid, block, 0, s, M, Xp, sl, Y, ldy, yin, ldin, beta, part); break;
  }
}

template <typename T>
void launch_sp_batch_cg_init(const SpBatchCgArgs<T> &a, hipStream_t s) {
  hipLaunchKernelGGL(sp_batch_cg_init_kernel<T>, dim3(a.bx + a.by, a.sl.nact), dim3(kVecTpb), 0, s, a);
}
template <typename T>
void launch_sp_batch_cg_xr(const SpBatchCgArgs<T> &a, hipStream_t s) {
  hipLaunchKernelGGL(sp_batch_cg_xr_kernel<T>, dim3(a.bx + a.by, a.sl.nact), dim3(kVecTpb), 0, s, a);
}
template <typename T>
void launch_sp_batch_cg_p(const SpBatchCgArgs<T> &a, hipStream_t s) {
  hipLaunchKernelGGL(sp_batch_cg_p_kernel<T>, dim3(a.bx, a.sl.nact), dim3(kVecTpb), 0, s, a);
}
template <typename T>
void launch_sp_batch_cg_close(const SpBatchCgArgs<T> &a, hipStream_t s) {
  hipLaunchKernelGGL(sp_batch_cg_close_kernel<T>, dim3(a.bx, a.sl.nact), dim3(kVecTpb), 0, s, a);
}
void launch_sp_batch_cg_scalars(int mode, const BatchSlots &sl, const double *sums, double *cg, double shift,
                                double eps, hipStream_t s) {
  hipLaunchKernelGGL(sp_batch_cg_scalars_kernel, dim3(1), dim3(64), 0, s, mode, sl, sums, cg, shift, eps);
}

template <typename T>
void sp_batch_spmv_check(int nrows, int ncols, const int *ptr, const int *ind, const T *val, int k, const int *act,
                         int nact, const T *X, size_t ldx, T beta, const T *yin, size_t ldin, T *Y, size_t ldy,
                         double *part, int num_cu, int *geom) {
  const BatchSlots sl = checked_batch_slots(k, act, nact);
  POGS_CHECK(nrows >= 1 && ncols >= 1, "nrows and ncols must be >= 1");
  POGS_CHECK(ptr && X && Y && geom, "null argument");
  POGS_CHECK(ptr[0] == 0, "ptr[0] must be 0");
  for (int r = 0; r < nrows; ++r) POGS_CHECK(ptr[r + 1] >= ptr[r], "CSR row pointers must not decrease");
  const size_t nnz = static_cast<size_t>(ptr[nrows]);
  POGS_CHECK(nnz == 0 || (ind && val), "null ind / val");
  for (size_t q = 0; q < nnz; ++q) POGS_CHECK(ind[q] >= 0 && ind[q] < ncols, "column index out of range [0, ncols)");
  POGS_CHECK(ldx >= static_cast<size_t>(ncols), "ldx must be >= ncols");
  POGS_CHECK(ldy >= static_cast<size_t>(nrows), "ldy must be >= nrows");
  POGS_CHECK(!yin || ldin >= static_cast<size_t>(nrows), "ldin must be >= nrows");
  POGS_CHECK(num_cu >= 0, "num_cu must be >= 0 (0: the device's)");
  int cu = num_cu;
  if (cu == 0) {
    int dev = 0;
    hipDeviceProp_t prop;
    POGS_HIP_CHECK(hipGetDevice(&dev));
    POGS_HIP_CHECK(hipGetDeviceProperties(&prop, dev));
    cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;   // (Ctx::init's)
  }
  const size_t nx = static_cast<size_t>(k) * ldx, ny = static_cast<size_t>(k) * ldy;
  const size_t nin = yin ? static_cast<size_t>(k) * ldin : 0;
  DevBuf<int> dptr(static_cast<size_t>(nrows) + 1), dind(std::max<size_t>(nnz, 1));
  DevBuf<T> dval(std::max<size_t>(nnz, 1)), dX(nx), dY(ny), dyin(nin),
      pk(static_cast<size_t>(ncols) * sp_batch_kp(sl.nact));
  POGS_HIP_CHECK(hipMemcpy(dptr.p, ptr, (static_cast<size_t>(nrows) + 1) * sizeof(int), hipMemcpyHostToDevice));
  if (nnz) {
    POGS_HIP_CHECK(hipMemcpy(dind.p, ind, nnz * sizeof(int), hipMemcpyHostToDevice));
    POGS_HIP_CHECK(hipMemcpy(dval.p, val, nnz * sizeof(T), hipMemcpyHostToDevice));
  }
  POGS_HIP_CHECK(hipMemcpy(dX.p, X, nx * sizeof(T), hipMemcpyHostToDevice));
  POGS_HIP_CHECK(hipMemcpy(dY.p, Y, ny * sizeof(T), hipMemcpyHostToDevice));
  if (yin) POGS_HIP_CHECK(hipMemcpy(dyin.p, yin, nin * sizeof(T), hipMemcpyHostToDevice));
  const SpBatchCsr<T> M = sp_batch_geometry(dval.p, dind.p, dptr.p, nrows, nnz, cu);
  const size_t npart = static_cast<size_t>(k) * M.grid;
  DevBuf<double> dpart(part ? npart : 0);
  if (part) POGS_HIP_CHECK(hipMemcpy(dpart.p, part, npart * sizeof(double), hipMemcpyHostToDevice));
  launch_sp_batch_pack<T>(dX.p, ldx, ncols, sl, pk.p, nullptr);
  launch_sp_batch_spmv<T>(M, pk.p, sl, dY.p, ldy, yin ? dyin.p : nullptr, ldin, beta, part ? dpart.p : nullptr, nullptr);
  POGS_HIP_CHECK(hipGetLastError());
  POGS_HIP_CHECK(hipMemcpy(Y, dY.p, ny * sizeof(T), hipMemcpyDeviceToHost));
  if (part) POGS_HIP_CHECK(hipMemcpy(part, dpart.p, npart * sizeof(double), hipMemcpyDeviceToHost));
  POGS_HIP_CHECK(hipDeviceSynchronize());
  geom[0] = M.lshift;
  geom[1] = M.rpw;
  geom[2] = M.grid;
}

#define POGS_SP_BATCH_INST(T)                                                                                          \
  template void launch_sp_batch_pack<T>(const T *, size_t, int, const BatchSlots &, T *, hipStream_t);                 \
  template void launch_sp_batch_spmv<T>(const SpBatchCsr<T> &, const T *, const BatchSlots &, T *, size_t, const T *,  \
                                        size_t, T, double *, hipStream_t);                                             \
  template void launch_sp_batch_cg_init<T>(const SpBatchCgArgs<T> &, hipStream_t);                                     \
  template void launch_sp_batch_cg_xr<T>(const SpBatchCgArgs<T> &, hipStream_t);                                       \
  template void launch_sp_batch_cg_p<T>(const SpBatchCgArgs<T> &, hipStream_t);                                        \
  template void launch_sp_batch_cg_close<T>(const SpBatchCgArgs<T> &, hipStream_t);                                   \
  template void sp_batch_spmv_check<T>(int, int, const int *, const int *, const T *, int, const int *, int,           \
                                       const T *, size_t, T, const T *, size_t, T *, size_t, double *, int, int *);
POGS_SP_BATCH_INST(float)
POGS_SP_BATCH_INST(double)

}  // namespace pogs_amd

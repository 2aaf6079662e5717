// Kernels of the batched sparse solves (sparse_batch.h): a multi-vector CSR product over the handle's equilibrated
// plain CSR copies (A and A^T), the pack of K operand vectors into one interleaved gather, and the batched CGLS
// vector stages.  Their own translation unit (sparse_batch_kernels.hip), so that the solo code objects stay as they
// are.  The element-wise ADMM stages are those of the shared loop (batch_admm.h, batch_kernels.h).
#pragma once
#include <hip/hip_runtime.h>

#include "batch_kernels.h"

namespace pogs_amd {

// The equilibrated CSR of one copy and its fixed product geometry: lanes per row (16 / 32 / 64) and rows per
// workgroup depend on the matrix only, so how a row's non-zeros are split over lanes, the reduction tree of its
// dot products and the order of the per-workgroup scalar records never depend on K or on the slot.
template <typename T>
struct SpBatchCsr {
  const T *val;
  const int *ind, *ptr;
  int nrows;
  int lshift;   // log2 of the lanes per row
  int rpw;      // rows per workgroup
  int grid;     // workgroups: ceil(nrows / rpw)
};
SpBatchCsr<float> sp_batch_geometry(const float *val, const int *ind, const int *ptr, int nrows, size_t nnz, int num_cu);
SpBatchCsr<double> sp_batch_geometry(const double *val, const int *ind, const int *ptr, int nrows, size_t nnz,
                                     int num_cu);

// operand slots per row of the interleaved layout: nact rounded up to 1 / 2 / 4 / 8 / 16
inline int sp_batch_kp(int nact) {
  int kp = 1;
  while (kp < nact) kp <<= 1;
  return kp;
}

// Xp[c * kp + slot] = X[act[slot] * ldx + c] for c < n (slots >= nact: zero)
template <typename T>
void launch_sp_batch_pack(const T *X, size_t ldx, int n, const BatchSlots &sl, T *Xp, hipStream_t s);
// Y[p * ldy + r] = (M Xp)[r][slot] (+ beta yin[p * ldin + r] when yin) for the problems p of sl; with part, the
// workgroup's sum of the squares of what it wrote goes to part[p * M.grid + workgroup] (one record per workgroup)
template <typename T>
void launch_sp_batch_spmv(const SpBatchCsr<T> &M, const T *Xp, const BatchSlots &sl, T *Y, size_t ldy, const T *yin,
                          size_t ldin, T beta, double *part, hipStream_t s);

// Diagnostic behind PogsAmdSpBatchSpmvCheck (HOST arrays; include/pogs_amd.h): argument checks, upload,
// sp_batch_geometry (num_cu = 0: the device's CU count), launch_sp_batch_pack, launch_sp_batch_spmv, download.
// geom = {lshift, rpw, grid}; part (may be null) receives k * grid doubles.
template <typename T>
void sp_batch_spmv_check(int nrows, int ncols, const int *ptr, const int *ind, const T *val, int k, const int *act,
                         int nact, const T *X, size_t ldx, T beta, const T *yin, size_t ldin, T *Y, size_t ldy,
                         double *part, int num_cu, int *geom);

// batched CGLS (cgls.h:200-323), one problem per grid row (slot).  cg: [kb][kSbCg] device scalars, sums: the
// problem's records of kBatchRec doubles (launch_batch_sums) at the slots of SpBatchSum
enum SpBatchSum : int { kSbQ2 = 0, kSbX2 = 1, kSbS2 = 2, kSbP2 = 3 };
enum SpBatchCg : int { kSbGamma = 0, kSbAlpha, kSbBeta, kSbDelta, kSbIndef, kSbCg = 8 };
template <typename T>
struct SpBatchCgArgs {
  int n, m, bx, by;
  size_t ldx, ldy;
  BatchSlots sl;
  const double *cg;
  T *x, *r, *p;             // CG state: x (n), r (m), p (n)
  const T *q, *sv;          // A p (m), A^T r - shift x (n)
  const T *x0, *y0, *xw, *yw;   // cg_init: x = xw - x0, r = y0 - yw; cg_close: x += x0
  double *part;             // [kb][bx] records of |x|^2 (xr) / |p|^2 (p)
  bool first;               // p stage: p = s
};
template <typename T> void launch_sp_batch_cg_init(const SpBatchCgArgs<T> &a, hipStream_t s);
template <typename T> void launch_sp_batch_cg_xr(const SpBatchCgArgs<T> &a, hipStream_t s);
template <typename T> void launch_sp_batch_cg_p(const SpBatchCgArgs<T> &a, hipStream_t s);
template <typename T> void launch_sp_batch_cg_close(const SpBatchCgArgs<T> &a, hipStream_t s);
// mode 0: gamma = |s|^2; 1: alpha = gamma / (|q|^2 + shift |p|^2); 2: beta = |s|^2 / gamma, gamma = |s|^2
void launch_sp_batch_cg_scalars(int mode, const BatchSlots &sl, const double *sums, double *cg, double shift,
                                double eps, hipStream_t s);

}  // namespace pogs_amd

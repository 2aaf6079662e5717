// Mixed storage (stream_mixed.h): the kernels of the fp64 one-pass iteration over the float copy of the matrix --
// the lean (one dot, one accumulator) and the full (two and two) form for FusedIterOp<double, false / true>, over the
// one-pass shapes of the mixed plan -- and the launch that rounds the equilibrated matrix.  One translation unit: the
// per-shape objects (dense_plan.hip) call the non-template launch functions and gain no kernel.
#include "stream_mixed.h"

namespace pogs_amd {

namespace {

template <typename Op>
void launch_mixed_t(const MixedPlan &p, bool full, const StreamArgsMixed &a, const Op &op, hipStream_t s) {
  POGS_CHECK(p.ok, "plan not supported by the mixed one-pass kernel");
  POGS_CHECK(a.n32 <= p.tpb * p.nv * 4 && a.n_pad <= a.n32 && a.n32 - a.n_pad <= 2 && a.n_pad % 2 == 0 && a.n32 % 4 == 0 &&
                 a.lda % 4 == 0 && a.lda >= static_cast<size_t>(a.n32),
             "mixed pass: the row does not fit the shape");
  const int grid = mixed_grid(p, full, a.m);
#define POGS_MIXED_CASE(TPB_, NV_)                                                                        \
  if constexpr (TPB_ <= 256)                                                                              \
  if (p.tpb == TPB_ && p.nv == NV_) {                                                                     \
    constexpr int T_ = mixed_exec_tpb(TPB_, NV_), V_ = mixed_exec_nv(TPB_, NV_);   /* the execution shape */ \
    if (full) {                                                                                           \
      constexpr int R_ = mixed_rows_c(T_, V_, 2);                                                         \
      static_assert(R_ >= 1, "the full form does not fit the register budget at this shape");             \
      const size_t lds = static_cast<size_t>(a.n32) * sizeof(double);                                     \
      static SmemGrants grants;   /* per device; concurrent solvers share it */                           \
      ensure_dynamic_smem(reinterpret_cast<const void *>(&stream_rows2_mixed_kernel<T_, V_, R_, 2, 2, Op>), lds, grants); \
      hipLaunchKernelGGL((stream_rows2_mixed_kernel<T_, V_, R_, 2, 2, Op>), dim3(grid), dim3(T_), lds, s, a, op); \
    } else {                                                                                              \
      constexpr int R_ = mixed_rows_c(T_, V_, 1);                                                         \
      static_assert(R_ >= 1, "the lean form does not fit the register budget at this shape");             \
      hipLaunchKernelGGL((stream_rows2_mixed_kernel<T_, V_, R_, 1, 1, Op>), dim3(grid), dim3(T_), 0, s, a, op); \
    }                                                                                                     \
    return;                                                                                               \
  }
  POGS_STREAM_PLANS(POGS_MIXED_CASE)
#undef POGS_MIXED_CASE
  throw Error("no mixed one-pass kernel for this shape");
}

// One element-wise pass: the narrow copy, and the wide one made equal to it.  Rounding is to nearest (the conversion's
// default); the row sums and d, e of the equilibration are not recomputed.
__global__ void __launch_bounds__(256) round_to_f32_kernel(double *A, size_t lda, float *A32, size_t lda32, int m, int n) {
  const int vpr = static_cast<int>(lda32 / 4);
  for (int row = blockIdx.x; row < m; row += gridDim.x) {
    double *rp = A + static_cast<size_t>(row) * lda;
    float *rq = A32 + static_cast<size_t>(row) * lda32;
    for (int v = threadIdx.x; v < vpr; v += 256) {
      float f[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int col = v * 4 + c;
        f[c] = 0.f;
        if (col < n) {
          f[c] = static_cast<float>(rp[col]);
          rp[col] = static_cast<double>(f[c]);
        }
      }
      *reinterpret_cast<float4 *>(rq + v * 4) = make_float4(f[0], f[1], f[2], f[3]);
    }
  }
}

}  // namespace

void launch_stream2_mixed(const MixedPlan &p, bool full, const StreamArgsMixed &a, const FusedIterOp<double, false> &op,
                          hipStream_t s) {
  launch_mixed_t(p, full, a, op, s);
}
void launch_stream2_mixed(const MixedPlan &p, bool full, const StreamArgsMixed &a, const FusedIterOp<double, true> &op,
                          hipStream_t s) {
  launch_mixed_t(p, full, a, op, s);
}

void launch_round_to_f32(double *A, size_t lda, float *A32, size_t lda32, int m, int n, int grid, hipStream_t s) {
  hipLaunchKernelGGL(round_to_f32_kernel, dim3(grid), dim3(256), 0, s, A, lda, A32, lda32, m, n);
}

}  // namespace pogs_amd

// Mixed storage on a fused-CGLS handle (stream_mixed.h): the instances of stream_rows_mixed_kernel -- the ACC-only,
// the DOT + ACC and the DOT-only pass over the float copy of the matrix, with the three functors the device-resident
// CGLS loop launches them with -- over the one-pass shapes of the mixed plan.  One translation unit: the per-shape
// objects (dense_plan.hip) and the diagnostic entry call the non-template launch functions and gain no kernel.
#include "stream_mixed.h"

namespace pogs_amd {

namespace {

template <bool DOT, bool ACC, typename Op>
void launch_mixed1_t(const MixedPlan &p, const StreamArgsMixed1 &a, const Op &op, hipStream_t s) {
  POGS_CHECK(p.ok, "plan not supported by the mixed streaming kernel");
  POGS_CHECK(a.m >= 1 && a.n32 >= 4 && a.n32 <= p.tpb * p.nv * 4 && a.n_pad <= a.n32 && a.n32 - a.n_pad <= 2 && a.n_pad % 2 == 0 &&
                 a.n32 % 4 == 0 && a.lda % 4 == 0 && a.lda >= static_cast<size_t>(a.n32),
             "mixed pass: the row does not fit the shape");
  const int grid = mixed1_grid(p, DOT, ACC, a.m);
#define POGS_MIXED1_CASE(TPB_, NV_)                                                                       \
  if constexpr (TPB_ <= 256)                                                                              \
  if (p.tpb == TPB_ && p.nv == NV_) {                                                                     \
    constexpr int T_ = mixed_exec_tpb(TPB_, NV_), V_ = mixed_exec_nv(TPB_, NV_);   /* the execution shape */ \
    constexpr int R_ = mixed1_rows_c(T_, V_, DOT, ACC);                                                   \
    static_assert(R_ >= 1, "the form does not fit the register budget at this shape");                    \
    hipLaunchKernelGGL((stream_rows_mixed_kernel<T_, V_, R_, DOT, ACC, Op>), dim3(grid), dim3(T_), 0, s, a, op); \
    return;                                                                                               \
  }
  POGS_STREAM_PLANS(POGS_MIXED1_CASE)
#undef POGS_MIXED1_CASE
  throw Error("no mixed streaming kernel for this shape");
}

}  // namespace

void launch_stream_mixed(const MixedPlan &p, const StreamArgsMixed1 &a, const GemvTOp<double> &op, hipStream_t s) {
  launch_mixed1_t<false, true>(p, a, op, s);
}
void launch_stream_mixed(const MixedPlan &p, const StreamArgsMixed1 &a, const DcgQRowOp<double> &op, hipStream_t s) {
  launch_mixed1_t<true, true>(p, a, op, s);
}
void launch_stream_mixed(const MixedPlan &p, const StreamArgsMixed1 &a, const ProjTailOp<double> &op, hipStream_t s) {
  launch_mixed1_t<true, false>(p, a, op, s);
}

}  // namespace pogs_amd

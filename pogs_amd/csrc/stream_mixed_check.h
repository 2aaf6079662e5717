#pragma once
// PogsAmdStreamMixedCheck (include/pogs_amd.h, Part 3): ONE launch of stream_rows_mixed_kernel (stream_mixed.h: the
// single-vector streaming pass over a FLOAT matrix with fp64 arithmetic) and its second stage -- reduce_cols of the
// column partials, the scalar records summed -- on HOST arrays, through the launch functions and with the functors the
// fused CGLS loop of a mixed-storage handle uses (dense_cg_fused.h): GemvTOp (ACC), DcgQRowOp (DOT + ACC, guarded),
// ProjTailOp (DOT).
//
// Contract of the matrix: rows of n32 = round_up(n, 4) floats at stride ldm; columns n .. n32 are zero; columns
// n32 .. ldm are never read.  x and tot have n_pad = round_up(n, 2) doubles: nothing at or past n_pad is read or
// written, also where the row's last float vector reaches past it.
#include <cstring>

#include "../../include/pogs_amd.h"
#include "common.h"
#include "ops.h"
#include "stream_mixed.h"
#include "vec_kernels.h"

namespace pogs_amd {

struct StreamMixedCheckArgs {
  int form, rows, n;
  const float *M;
  size_t ldm;
  int num_cu, force_tpb, force_nv;
  const double *x, *u;
  double done;
  double *q, *tot, *scalars, *partials;
  size_t partials_len;
  int *info;
};

inline MixedPlan stream_mixed_check_plan(const StreamMixedCheckArgs &a, int num_cu) {
  return a.force_tpb != 0 ? mixed_plan_of_shape(a.force_tpb, a.force_nv, num_cu) : make_mixed_plan(static_cast<size_t>(a.n), num_cu);
}

// every refusal, before any device work; the messages name the argument
inline void stream_mixed_check_validate(const StreamMixedCheckArgs &a) {
  POGS_CHECK(a.form == POGS_AMD_STREAM_MIXED_ACC || a.form == POGS_AMD_STREAM_MIXED_DOT_ACC || a.form == POGS_AMD_STREAM_MIXED_DOT,
             "form must be ACC, DOT_ACC or DOT");
  POGS_CHECK(a.rows >= 1 && a.n >= 1, "rows and n must be >= 1");
  POGS_CHECK(a.M && a.info, "null argument: M, info");
  const size_t n32 = round_up(static_cast<size_t>(a.n), 4);
  POGS_CHECK(a.ldm % 4 == 0 && a.ldm >= n32, "ldm must be a multiple of 4 and >= round_up(n, 4)");
  POGS_CHECK(a.num_cu >= 0 && a.num_cu <= 1024, "num_cu must be in [0, 1024]");
  if (a.force_tpb != 0 || a.force_nv != 0) {
    POGS_CHECK(mixed_shape_listed(a.force_tpb, a.force_nv), "force_tpb, force_nv: not a one-pass shape of the mixed plan");
    POGS_CHECK(static_cast<size_t>(a.force_tpb) * a.force_nv * 4 >= n32, "force_tpb, force_nv: the shape does not hold round_up(n, 4)");
  }
  POGS_CHECK(stream_mixed_check_plan(a, 1).ok, "n: the row fits no one-pass shape of the mixed plan (n <= 10240, not windowed)");
  const bool dot = a.form != POGS_AMD_STREAM_MIXED_ACC, acc = a.form != POGS_AMD_STREAM_MIXED_DOT;
  if (dot) POGS_CHECK(a.x && a.q && a.scalars, "null argument: x, q, scalars (forms DOT_ACC and DOT)");
  if (!dot) POGS_CHECK(a.u != nullptr, "null argument: u (form ACC)");
  if (acc) POGS_CHECK(a.tot != nullptr, "null argument: tot (forms ACC and DOT_ACC)");
  POGS_CHECK(!a.partials || acc, "partials: form DOT forms no column partials");
}

inline void stream_mixed_check_run(const StreamMixedCheckArgs &a, int num_cu) {
  hipStream_t s = nullptr;
  const int rows = a.rows, n = a.n;
  const int n_pad = static_cast<int>(round_up(static_cast<size_t>(n), 2)), n32 = static_cast<int>(round_up(static_cast<size_t>(n), 4));
  const MixedPlan p = stream_mixed_check_plan(a, num_cu);
  const bool dot = a.form != POGS_AMD_STREAM_MIXED_ACC, acc = a.form != POGS_AMD_STREAM_MIXED_DOT;
  const int grid = mixed1_grid(p, dot, acc, rows), R = mixed1_rows(p, dot, acc);
  const size_t part_count = static_cast<size_t>(grid) * n_pad;
  POGS_CHECK(!a.partials || a.partials_len >= part_count, "partials_len must be >= grid * round_up(n, 2)");

  // device copies: inputs uploaded, outputs uploaded too (what no launch writes comes back as it was)
  auto up = [](DevBuf<double> &d, const void *h, size_t cnt) {
    d.alloc(cnt);
    if (h) POGS_HIP_CHECK(hipMemcpy(d.p, h, cnt * sizeof(double), hipMemcpyHostToDevice));
    else POGS_HIP_CHECK(hipMemset(d.p, 0, cnt * sizeof(double)));
  };
  DevBuf<float> dM(static_cast<size_t>(rows) * a.ldm);
  POGS_HIP_CHECK(hipMemcpy(dM.p, a.M, dM.n * sizeof(float), hipMemcpyHostToDevice));
  DevBuf<double> x, u, q, tot, zero_rows, ztemp, S(kNumSlots), Sout(2);
  up(x, a.x, n_pad); up(u, a.u, rows); up(q, a.q, rows); up(tot, a.tot, n_pad);
  up(zero_rows, nullptr, rows); up(ztemp, nullptr, rows);
  up(Sout, a.scalars, 2);
  S.zero(s);
  POGS_HIP_CHECK(hipMemcpy(S.p + kFcDone, &a.done, sizeof(double), hipMemcpyHostToDevice));
  // partial sums start as NaN: a slot no workgroup wrote shows in every total that reads it
  DevBuf<double> part(part_count), spart(static_cast<size_t>(grid) * 2 + static_cast<size_t>(reduce_cols_grid(n_pad, 2)) * 4);
  POGS_HIP_CHECK(hipMemset(part.p, 0xFF, part_count * sizeof(double)));
  POGS_HIP_CHECK(hipMemset(spart.p, 0xFF, spart.n * sizeof(double)));
  double *sp = spart.p + static_cast<size_t>(grid) * 2;

  const StreamArgsMixed1 am{dM.p, a.ldm, rows, n_pad, n32, x.p, part.p, spart.p};
  int ns = 0;
  bool ran = true;
  if (a.form == POGS_AMD_STREAM_MIXED_ACC) {
    launch_stream_mixed(p, am, GemvTOp<double>{1, u.p}, s);
  } else if (a.form == POGS_AMD_STREAM_MIXED_DOT_ACC) {
    launch_stream_mixed(p, am, DcgQRowOp<double>{q.p, S.p}, s);
    ns = 1;
    ran = a.done == 0.0;   // (an ended loop: the second stage returns at the same flag, dcg_step_a_kernel)
  } else {
    launch_stream_mixed(p, am, ProjTailOp<double>{q.p, zero_rows.p, zero_rows.p, ztemp.p}, s);
    ns = 2;
  }
  if (ran && ns > 0) {
    const SumJob j{spart.p, grid, ns, Sout.p};
    launch_sum_jobs(&j, 1, s);
  }
  if (ran && acc) launch_reduce_cols<double, StoreColOp<double>>(part.p, grid, n_pad, StoreColOp<double>{1, 0, tot.p, n}, sp, s);
  POGS_HIP_CHECK(hipGetLastError());
  POGS_HIP_CHECK(hipDeviceSynchronize());
  auto down = [](void *h, const DevBuf<double> &d, size_t cnt) {
    if (h) POGS_HIP_CHECK(hipMemcpy(h, d.p, cnt * sizeof(double), hipMemcpyDeviceToHost));
  };
  down(a.q, q, rows); down(a.tot, tot, n_pad); down(a.scalars, Sout, 2);
  if (a.partials) down(a.partials, part, part_count);
  const int et = mixed_exec_tpb(p.tpb, p.nv), ev = mixed_exec_nv(p.tpb, p.nv);
  const int out[8] = {p.tpb, p.nv, R, grid, et, ev, ns, mixed1_blocks_per_cu(et, ev, dot, acc)};
  for (int i = 0; i < 8; ++i) a.info[i] = out[i];
}

}  // namespace pogs_amd

#pragma once
// PogsAmdDensePassMixedCheck (include/pogs_amd.h, Part 3): ONE mixed-storage pass (stream_mixed.h: the fp64 one-pass
// iteration's pass over a FLOAT matrix) and its second stage on HOST arrays, through the launch functions a
// POGS_AMD_STORE_F32 handle calls.  The struct, the second stages and the outputs are those of PogsAmdDensePassCheck
// (pass_check.h) with T = double for every vector; M alone is float.
//
// Contract of the stored matrix: rows of n32 = round_up(n, 4) floats at stride ldm; columns n .. n32 are zero; columns
// n32 .. ldm are never read.  The vectors have n_pad = round_up(n, 2) entries: of the dot vectors and of a partial-sum
// record nothing at or past n_pad is read or written, also where the row's last float vector reaches past it.
#include <cstring>

#include "../../include/pogs_amd.h"
#include "common.h"
#include "fused_cols.h"
#include "ops.h"
#include "stream_mixed.h"
#include "vec_kernels.h"

namespace pogs_amd {

inline MixedPlan pass_mixed_check_plan(const PogsAmdDensePassArgs &a, int num_cu) {
  return a.force_tpb != 0 ? mixed_plan_of_shape(a.force_tpb, a.force_nv, num_cu) : make_mixed_plan(static_cast<size_t>(a.n), num_cu);
}

// every refusal, before any device work; the messages name the argument
inline void pass_mixed_check_validate(const PogsAmdDensePassArgs &a) {
  POGS_CHECK(a.dtype == POGS_AMD_F64, "dtype must be POGS_AMD_F64 (the mixed pass is an fp64 pass over a float matrix)");
  POGS_CHECK(a.form == POGS_AMD_PASS_ITER_FULL || a.form == POGS_AMD_PASS_ITER_LEAN, "form must be ITER_FULL or ITER_LEAN");
  POGS_CHECK(a.functor == POGS_AMD_PASS_FN_CHEAP || a.functor == POGS_AMD_PASS_FN_LOGISTIC, "functor must be CHEAP or LOGISTIC");
  POGS_CHECK(a.cols >= POGS_AMD_PASS_COLS_REDUCE && a.cols <= POGS_AMD_PASS_COLS_PACK, "unknown cols");
  POGS_CHECK(a.rows >= 1 && a.n >= 1, "rows and n must be >= 1");
  POGS_CHECK(a.M && a.info, "null argument: M, info");
  const size_t n_pad = round_up(static_cast<size_t>(a.n), 2), n32 = round_up(static_cast<size_t>(a.n), 4);
  POGS_CHECK(a.ldm % 4 == 0 && a.ldm >= n32, "ldm must be a multiple of 4 and >= round_up(n, 4)");
  POGS_CHECK(a.num_cu >= 0 && a.num_cu <= 1024, "num_cu must be in [0, 1024]");
  POGS_CHECK(a.row_len >= static_cast<size_t>(a.rows), "row_len must be >= rows");
  POGS_CHECK(a.col_len >= n_pad, "col_len must be >= n_pad");
  POGS_CHECK(a.dots == nullptr, "dots must be NULL (the plain row-dot launch has no mixed form)");
  if (a.force_tpb != 0 || a.force_nv != 0) {
    POGS_CHECK(mixed_shape_listed(a.force_tpb, a.force_nv), "force_tpb, force_nv: not a one-pass shape of the mixed plan");
    POGS_CHECK(static_cast<size_t>(a.force_tpb) * a.force_nv * 4 >= n32, "force_tpb, force_nv: the shape does not hold round_up(n, 4)");
  }
  POGS_CHECK(pass_mixed_check_plan(a, 1).ok, "n: the row fits no one-pass shape of the mixed plan (n <= 10240, not windowed)");
  const bool lean = a.form == POGS_AMD_PASS_ITER_LEAN;
  POGS_CHECK(a.ytemp && a.y12, "null argument: ytemp, y12");
  POGS_CHECK(a.x0 && (lean || a.x1), "null argument: x0, x1");
  POGS_CHECK(a.ycur && a.ynew && a.y12s && a.ytemps && a.scalars, "null argument: ycur, ynew, y12s, ytemps, scalars");
  POGS_CHECK(a.f_h && a.f_a && a.f_b && a.f_c && a.f_d && a.f_e, "null argument: f_h, f_a .. f_e");
  switch (a.cols) {
    case POGS_AMD_PASS_COLS_REDUCE:
      POGS_CHECK(a.tot0 && (lean || a.tot1), "null argument: tot0, tot1");
      break;
    case POGS_AMD_PASS_COLS_PACK:
      POGS_CHECK(!lean, "cols PACK: a lean pass forms one partial set (REDUCE or PRE_ONE)");
      POGS_CHECK(a.pack, "null argument: pack");
      break;
    default:
      POGS_CHECK(!(lean && a.cols == POGS_AMD_PASS_COLS_PRE), "cols PRE: a lean pass forms one partial set (REDUCE or PRE_ONE)");
      POGS_CHECK(a.g_h && a.g_a && a.g_b && a.g_c && a.g_d && a.g_e, "null argument: g_h, g_a .. g_e");
      POGS_CHECK(a.x_cur && a.xt && a.x12 && a.xtemp && a.rhs && a.col_scalars, "null argument: x_cur, xt, x12, xtemp, rhs, col_scalars");
  }
}

inline void pass_mixed_check_run(const PogsAmdDensePassArgs &a, int num_cu) {
  using T = double;
  hipStream_t s = nullptr;
  const int rows = a.rows, n = a.n;
  const int n_pad = static_cast<int>(round_up(static_cast<size_t>(n), 2)), n32 = static_cast<int>(round_up(static_cast<size_t>(n), 4));
  const MixedPlan p = pass_mixed_check_plan(a, num_cu);
  const bool full = a.form == POGS_AMD_PASS_ITER_FULL, lean = !full;
  const int grid = mixed_grid(p, full, rows), R = mixed_rows(p, full), nparts = grid;

  // device copies: inputs uploaded, outputs uploaded too (what no launch writes comes back as it was)
  auto up = [](DevBuf<T> &d, const void *h, size_t cnt) {
    if (!h) return;
    d.alloc(cnt);
    POGS_HIP_CHECK(hipMemcpy(d.p, h, cnt * sizeof(T), hipMemcpyHostToDevice));
  };
  auto down = [](void *h, const DevBuf<T> &d) {
    if (h && d.p) POGS_HIP_CHECK(hipMemcpy(h, d.p, d.n * sizeof(T), hipMemcpyDeviceToHost));
  };
  auto up_fn = [](FnBuf<T> &d, const int *h, const void *fa, const void *fb, const void *fc, const void *fd, const void *fe, size_t cnt) {
    if (!h) return;
    d.alloc(cnt);
    POGS_HIP_CHECK(hipMemcpy(d.h.p, h, cnt * sizeof(int), hipMemcpyHostToDevice));
    const void *src[5] = {fa, fb, fc, fd, fe};
    T *dst[5] = {d.a.p, d.b.p, d.c.p, d.d.p, d.e.p};
    for (int k = 0; k < 5; ++k) POGS_HIP_CHECK(hipMemcpy(dst[k], src[k], cnt * sizeof(T), hipMemcpyHostToDevice));
  };
  DevBuf<float> dM(static_cast<size_t>(rows) * a.ldm);
  POGS_HIP_CHECK(hipMemcpy(dM.p, a.M, dM.n * sizeof(float), hipMemcpyHostToDevice));
  DevBuf<T> x0, x1, ycur, y12, ytemp, ynew, y12s, ytemps, tot0, tot1, x_cur, xt, x12, xtemp, rhs;
  FnBuf<T> f, g;
  up(x0, a.x0, a.col_len); up(x1, a.x1, a.col_len);
  up(ycur, a.ycur, a.row_len); up(y12, a.y12, a.row_len); up(ytemp, a.ytemp, a.row_len);
  up(ynew, a.ynew, a.row_len); up(y12s, a.y12s, a.row_len); up(ytemps, a.ytemps, a.row_len);
  up(tot0, a.tot0, a.col_len); up(tot1, a.tot1, a.col_len);
  up(x_cur, a.x_cur, a.col_len); up(xt, a.xt, a.col_len); up(x12, a.x12, a.col_len); up(xtemp, a.xtemp, a.col_len);
  up(rhs, a.rhs, a.col_len);
  up_fn(f, a.f_h, a.f_a, a.f_b, a.f_c, a.f_d, a.f_e, a.row_len);
  up_fn(g, a.g_h, a.g_a, a.g_b, a.g_c, a.g_d, a.g_e, a.col_len);
  const size_t pack_count = 2 * static_cast<size_t>(n_pad) + 6;
  DevBuf<double> pack;
  if (a.pack) {
    pack.alloc(pack_count);
    POGS_HIP_CHECK(hipMemcpy(pack.p, a.pack, pack_count * sizeof(double), hipMemcpyHostToDevice));
  }
  // partial sums start as NaN: a slot no workgroup wrote shows in every total that reads it
  const size_t part_count = static_cast<size_t>(nparts) * n_pad;
  DevBuf<T> part0(part_count), part1(part_count);
  POGS_HIP_CHECK(hipMemset(part0.p, 0xFF, part_count * sizeof(T)));
  POGS_HIP_CHECK(hipMemset(part1.p, 0xFF, part_count * sizeof(T)));
  const int gridR = reduce_cols_grid(n_pad, 2), gridC = pre_cols_grid(n_pad, 2);
  const size_t sp_row = static_cast<size_t>(grid) * 6, sp_col = static_cast<size_t>(gridR > gridC ? gridR : gridC) * 4;
  DevBuf<double> spart(sp_row + sp_col), S(16);
  POGS_HIP_CHECK(hipMemset(spart.p, 0xFF, spart.n * sizeof(double)));
  S.zero(s);
  double *sp = spart.p + sp_row;

  const T rho = a.rho, alpha = a.alpha, zs = a.zs;
  const SumJob jd{spart.p, grid, 3, S.p, 6, 0}, js{spart.p, grid, 3, S.p + 3, 6, 3};
  const StreamArgsMixed am{dM.p, a.ldm, rows, n_pad, n32, x0.p, x1.p, part0.p, part1.p, spart.p};
  if (a.functor == POGS_AMD_PASS_FN_LOGISTIC) {
    launch_stream2_mixed(p, full, am, FusedIterOp<T, true>{ynew.p, ycur.p, y12.p, ytemp.p, f.view(), rho, alpha, zs, y12s.p, ytemps.p}, s);
  } else {
    launch_stream2_mixed(p, full, am, FusedIterOp<T, false>{ynew.p, ycur.p, y12.p, ytemp.p, f.view(), rho, alpha, zs, y12s.p, ytemps.p}, s);
  }
  {
    const SumJob j[2] = {jd, js};
    launch_sum_jobs(j, 2, s);
  }
  if (a.cols == POGS_AMD_PASS_COLS_REDUCE) {
    launch_reduce_cols<T, StoreColOp<T>>(part0.p, nparts, n_pad, StoreColOp<T>{1, 0, tot0.p, n}, sp, s);
    if (!lean) launch_reduce_cols<T, StoreColOp<T>>(part1.p, nparts, n_pad, StoreColOp<T>{1, 0, tot1.p, n}, sp, s);
  } else if (a.cols == POGS_AMD_PASS_COLS_PACK) {
    PackJobs pj;
    pj.j[0] = jd; pj.j[1] = js; pj.njobs = 2;
    launch_pack_cols<T>(part0.p, part1.p, nparts, n_pad, pack.p, pj, s);
  } else {
    PreColsArgs<T> pc;
    pc.part0 = part0.p; pc.part1 = a.cols == POGS_AMD_PASS_COLS_PRE_ONE ? nullptr : part1.p; pc.nparts = nparts;
    pc.tot64 = nullptr;
    pc.n = n; pc.n_pad = n_pad;
    pc.g = g.view();
    pc.x_cur = x_cur.p; pc.xt = xt.p;
    pc.zt_scale = zs; pc.rho = rho; pc.alpha = alpha;
    pc.x12 = x12.p; pc.xtemp = xtemp.p; pc.rhs = rhs.p;
    pc.partials = sp;
    launch_pre_cols<T>(pc, false, s);
    const SumJob j[2] = {{sp, gridC, 3, S.p + 8, 4, 0}, {sp, gridC, 1, S.p + 11, 4, 3}};
    launch_sum_jobs(j, 2, s);
  }
  POGS_HIP_CHECK(hipGetLastError());
  POGS_HIP_CHECK(hipDeviceSynchronize());
  down(a.ytemp, ytemp); down(a.ynew, ynew); down(a.y12s, y12s); down(a.ytemps, ytemps);
  down(a.tot0, tot0); down(a.tot1, tot1);
  down(a.x12, x12); down(a.xtemp, xtemp); down(a.rhs, rhs);
  if (a.pack) POGS_HIP_CHECK(hipMemcpy(a.pack, pack.p, pack_count * sizeof(double), hipMemcpyDeviceToHost));
  double Sh[16];
  POGS_HIP_CHECK(hipMemcpy(Sh, S.p, sizeof(Sh), hipMemcpyDeviceToHost));
  if (a.scalars) std::memcpy(a.scalars, Sh, 6 * sizeof(double));
  if (a.col_scalars) std::memcpy(a.col_scalars, Sh + 8, 4 * sizeof(double));
  const int out[8] = {p.tpb, p.nv, R, grid, 1, 3, nparts, 0};
  for (int i = 0; i < 8; ++i) a.info[i] = out[i];
}

}  // namespace pogs_amd

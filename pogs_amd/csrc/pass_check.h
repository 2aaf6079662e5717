#pragma once
// PogsAmdDensePassCheck (include/pogs_amd.h, Part 3): ONE dense streaming pass and its second stage on HOST arrays,
// through the launch functions a dense solve calls, with the functors and forms it instantiates -- so the per-shape
// objects (dense_plan.hip) gain no kernel.  abi.hip runs the refusals (no device needed) and picks the object;
// dense_pass_check_t runs in that object.
//
// Contract of the stored matrix (stream.h), which the tests poison around:
//   * rows of n_pad = round_up(n, VEC) elements at stride ldm; columns n .. n_pad of M and entries n .. n_pad of the dot
//     vectors are zero; columns n_pad .. ldm are never read;
//   * kLower (W_SWEEP): of row i the vectors 0 .. i / VEC are loaded WHOLE, the one holding the diagonal included, so the
//     entries right of the diagonal inside that vector must be zero (the factor's slab is zeroed before L^-1 is written);
//     vectors wholly right of the diagonal are not loaded.  kUpper mirrors it: the vector holding the diagonal is loaded
//     whole, entries left of the diagonal inside it must be zero.
#include <cstring>
#include <type_traits>

#include "../../include/pogs_amd.h"
#include "common.h"
#include "fused_cols.h"
#include "ops.h"
#include "stream.h"
#include "vec_kernels.h"

namespace pogs_amd {

inline bool pass_shape_listed(int tpb, int nv) {
#define POGS_PASS_LISTED(TPB_, NV_) if (tpb == TPB_ && nv == NV_) return true;
  POGS_STREAM_PLANS(POGS_PASS_LISTED)
#undef POGS_PASS_LISTED
  return false;
}

// the shape and its per-solve tuning, as a solve of these functions would run it
template <typename T>
inline StreamPlan pass_check_plan(const PogsAmdDensePassArgs &a, int num_cu) {
  const int n_pad = static_cast<int>(round_up(static_cast<size_t>(a.n), Vec16<T>::N));
  StreamPlan p = a.force_tpb != 0 ? stream_plan_of_shape(a.force_tpb, a.force_nv, num_cu) : make_stream_plan<T>(n_pad, num_cu);
  const bool iter = a.form == POGS_AMD_PASS_ITER_FULL || a.form == POGS_AMD_PASS_ITER_LEAN;
  tune_stream_plan<T>(p, iter, iter && a.functor == POGS_AMD_PASS_FN_LOGISTIC, a.functor == POGS_AMD_PASS_FN_XSIDE);
  return p;
}

// every refusal, before any device work; the messages name the argument
inline void pass_check_validate(const PogsAmdDensePassArgs &a) {
  POGS_CHECK(a.dtype == POGS_AMD_F32 || a.dtype == POGS_AMD_F64, "unknown dtype");
  const bool f32 = a.dtype == POGS_AMD_F32;
  const size_t VEC = f32 ? 4 : 2;
  POGS_CHECK(a.form >= POGS_AMD_PASS_PRE_ACC && a.form <= POGS_AMD_PASS_W_SWEEP, "unknown form");
  POGS_CHECK(a.functor >= POGS_AMD_PASS_FN_CHEAP && a.functor <= POGS_AMD_PASS_FN_XSIDE, "unknown functor");
  POGS_CHECK(a.cols >= POGS_AMD_PASS_COLS_REDUCE && a.cols <= POGS_AMD_PASS_COLS_PACK, "unknown cols");
  POGS_CHECK(a.rows >= 1 && a.n >= 1, "rows and n must be >= 1");
  POGS_CHECK(a.M && a.info, "null argument: M, info");
  const size_t n_pad = round_up(static_cast<size_t>(a.n), VEC);
  POGS_CHECK(a.ldm % VEC == 0 && a.ldm >= n_pad, "ldm must be a multiple of VEC and >= n_pad");
  POGS_CHECK(a.num_cu >= 0 && a.num_cu <= 1024, "num_cu must be in [0, 1024]");
  POGS_CHECK(a.row_len >= static_cast<size_t>(a.rows), "row_len must be >= rows");
  POGS_CHECK(a.col_len >= n_pad, "col_len must be >= n_pad");
  if (a.force_tpb != 0 || a.force_nv != 0) {
    POGS_CHECK(pass_shape_listed(a.force_tpb, a.force_nv), "force_tpb, force_nv: not a shape of POGS_STREAM_PLANS");
    POGS_CHECK(static_cast<size_t>(a.force_tpb) * a.force_nv * VEC >= n_pad, "force_tpb, force_nv: the shape does not hold n_pad");
  }
  const bool lean = a.form == POGS_AMD_PASS_ITER_LEAN, full = a.form == POGS_AMD_PASS_ITER_FULL;
  const bool pre = a.form == POGS_AMD_PASS_PRE_ACC;
  POGS_CHECK(!(lean && f32), "form ITER_LEAN is built for fp64 only (dense_iter.h: kLeanType)");
  POGS_CHECK(!(lean && a.functor == POGS_AMD_PASS_FN_XSIDE), "functor XSIDE has no lean form");
  POGS_CHECK(!(pre && a.functor == POGS_AMD_PASS_FN_LOGISTIC), "functor LOGISTIC: form PRE_ACC takes CHEAP (PreAccOp) or XSIDE (PreAcc2Op)");
  const StreamPlan p = f32 ? pass_check_plan<float>(a, 1) : pass_check_plan<double>(a, 1);
  POGS_CHECK(p.ok, "no streaming shape for n");
  if (pre || full || lean) {
    POGS_CHECK(stream2_supported(p), "form: the one-pass kernels run on no windowed and no 1024-thread shape");
    POGS_CHECK(a.ytemp && a.y12, "null argument: ytemp, y12");
    POGS_CHECK(!(pre && a.functor == POGS_AMD_PASS_FN_CHEAP) || (a.yt && a.ycur), "null argument: yt, ycur");
    if (full || lean) {
      POGS_CHECK(a.x0 && (lean || a.x1), "null argument: x0, x1");
      POGS_CHECK(a.ycur && a.ynew && a.y12s && a.ytemps && a.scalars, "null argument: ycur, ynew, y12s, ytemps, scalars");
      POGS_CHECK(a.f_h && a.f_a && a.f_b && a.f_c && a.f_d && a.f_e, "null argument: f_h, f_a .. f_e");
      POGS_CHECK(a.functor != POGS_AMD_PASS_FN_XSIDE || a.yt, "null argument: yt (XSIDE: the old dual vector)");
    }
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
  } else if (a.form == POGS_AMD_PASS_EXACT) {
    POGS_CHECK(a.x0 && a.y12 && a.yt && a.ycur && a.scalars, "null argument: x0, y12, yt, ycur, scalars");
    POGS_CHECK(a.x12 && a.xt && a.x_cur && a.col_scalars && a.tot0, "null argument: x12, xt, x_cur, col_scalars, tot0");
  } else {
    POGS_CHECK(a.rows == a.n, "form W_SWEEP needs rows == n (a square lower-triangular M)");
    POGS_CHECK(a.x0 && a.tot0, "null argument: x0, tot0");
  }
}

template <typename T, typename Tag, typename Op>
inline void pass_check_iter(const StreamPlan &p, const StreamArgs2<T> &a2, const Op &op, bool full, hipStream_t s) {
  if (full) {
    launch_stream2<T, 2, 2, Tag>(p, a2, op, s);
    return;
  }
  if constexpr (std::is_same<T, double>::value) launch_stream2<T, 1, 1, Tag>(p, a2, op, s);
  else throw Error("form ITER_LEAN is built for fp64 only (dense_iter.h: kLeanType)");
}

template <typename T, typename Tag>
void dense_pass_check_t(const PogsAmdDensePassArgs &a, int num_cu) {
  constexpr int VEC = Vec16<T>::N;
  hipStream_t s = nullptr;
  const int rows = a.rows, n = a.n, n_pad = static_cast<int>(round_up(static_cast<size_t>(n), VEC));
  const StreamPlan p = pass_check_plan<T>(a, num_cu);
  POGS_CHECK(p.xl ? Tag::windows : Tag::has(p.tpb, p.nv), "dense pass check built for another streaming shape (abi.hip)");
  const bool full = a.form == POGS_AMD_PASS_ITER_FULL, lean = a.form == POGS_AMD_PASS_ITER_LEAN, iter = full || lean;
  const bool pre = a.form == POGS_AMD_PASS_PRE_ACC, exact = a.form == POGS_AMD_PASS_EXACT, sweep = a.form == POGS_AMD_PASS_W_SWEEP;
  // what the launch functions below will choose (stream.h: stream2_grid / stream_grid, launch_stream2's prefetching
  // case, launch_stream_plain's triangular case), restated for info and for the sizes of the partial-sum buffers
  int grid = 0, R = 0, kernel = 0;
  if (pre) { grid = stream2_grid<0>(p, rows); R = stream2_rows<0>(p); }
  else if (full) { grid = stream2_grid<2>(p, rows); R = stream2_rows<2>(p); kernel = (p.pf && std::is_same<T, float>::value) ? 2 : 0; }
  else if (lean) { grid = stream2_grid<1, 1>(p, rows); R = stream2_rows<1, 1>(p); }
  else {
    grid = stream_grid<true, true>(p, rows);
    R = p.tpb == 1024 ? 1 : 2;
    kernel = (sweep && !p.xl && !(p.tpb == 1024 && p.nv == 8)) ? 1 : 0;
  }
  const int nparts = grid;

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
  DevBuf<T> dM, x0, x1, ycur, y12, yt, ytemp, ynew, y12s, ytemps, dots, tot0, tot1, x_cur, xt, x12, xtemp, rhs;
  FnBuf<T> f, g;
  up(dM, a.M, static_cast<size_t>(rows) * a.ldm);
  up(x0, a.x0, a.col_len); up(x1, a.x1, a.col_len);
  up(ycur, a.ycur, a.row_len); up(y12, a.y12, a.row_len); up(yt, a.yt, a.row_len); up(ytemp, a.ytemp, a.row_len);
  up(ynew, a.ynew, a.row_len); up(y12s, a.y12s, a.row_len); up(ytemps, a.ytemps, a.row_len); up(dots, a.dots, 2 * a.row_len);
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
  const int gridR = reduce_cols_grid(n_pad, VEC), gridC = pre_cols_grid(n_pad, VEC);
  const size_t sp_row = static_cast<size_t>(grid) * 6, sp_col = static_cast<size_t>(gridR > gridC ? gridR : gridC) * 4;
  DevBuf<double> spart(sp_row + 2 * sp_col), S(16);
  POGS_HIP_CHECK(hipMemset(spart.p, 0xFF, spart.n * sizeof(double)));
  S.zero(s);
  double *sp = spart.p + sp_row, *sp2 = sp + sp_col;
  DevBuf<T> xl(stream_xl_scratch<T>(p, rows, n_pad));

  StreamArgs<T> sa;
  sa.A = dM.p; sa.lda = a.ldm; sa.m = rows; sa.n_pad = n_pad;
  sa.xin = x0.p; sa.xin_add = nullptr; sa.xin_nrm2 = nullptr;
  sa.col_partials = nullptr; sa.scalar_partials = spart.p;
  sa.xl_scratch = xl.p;
  if (a.dots) {   // the plain row dots, by the solver's row-dot launch (PogsAmdMul / the first product of solve_gram)
    if (sweep) {
      sa.xin_add = x1.p;
      launch_stream<T, true, false, false, kLower, Tag>(p, sa, GemvNOp<T>{1, 0, dots.p}, s);
    } else if (x0.p) {
      launch_stream<T, true, false, false, kFull, Tag>(p, sa, GemvNOp<T>{1, 0, dots.p}, s);
      if (x1.p) {
        sa.xin = x1.p;
        launch_stream<T, true, false, false, kFull, Tag>(p, sa, GemvNOp<T>{1, 0, dots.p + a.row_len}, s);
        sa.xin = x0.p;
      }
    }
  }
  sa.col_partials = part0.p;
  const T rho = static_cast<T>(a.rho), alpha = static_cast<T>(a.alpha), zs = static_cast<T>(a.zs), c_old = static_cast<T>(a.c_old);
  const SumJob jd{spart.p, grid, 3, S.p, 6, 0}, js{spart.p, grid, 3, S.p + 3, 6, 3};
  if (pre || iter) {
    StreamArgs2<T> a2{dM.p, a.ldm, rows, n_pad, iter ? x0.p : nullptr, iter ? x1.p : nullptr, part0.p, part1.p, spart.p};
    if (pre) {
      if (a.functor == POGS_AMD_PASS_FN_CHEAP) launch_stream2<T, 0, 2, Tag>(p, a2, PreAccOp<T>{ytemp.p, y12.p, yt.p, ycur.p, zs}, s);
      else launch_stream2<T, 0, 2, Tag>(p, a2, PreAcc2Op<T>{ytemp.p, y12.p}, s);
    } else {
      if (a.functor == POGS_AMD_PASS_FN_XSIDE) {
        FusedIterOp<T, false, true> op{ynew.p, ycur.p, y12.p, ytemp.p, f.view(), rho, alpha, zs, y12s.p, ytemps.p, yt.p, c_old};
        launch_stream2<T, 2, 2, Tag>(p, a2, op, s);
      } else if (a.functor == POGS_AMD_PASS_FN_LOGISTIC) {
        FusedIterOp<T, true> op{ynew.p, ycur.p, y12.p, ytemp.p, f.view(), rho, alpha, zs, y12s.p, ytemps.p};
        pass_check_iter<T, Tag>(p, a2, op, full, s);
      } else {
        FusedIterOp<T, false> op{ynew.p, ycur.p, y12.p, ytemp.p, f.view(), rho, alpha, zs, y12s.p, ytemps.p};
        pass_check_iter<T, Tag>(p, a2, op, full, s);
      }
      const SumJob j[2] = {jd, js};
      launch_sum_jobs(j, 2, s);
    }
    if (a.cols == POGS_AMD_PASS_COLS_REDUCE) {
      launch_reduce_cols<T, StoreColOp<T>>(part0.p, nparts, n_pad, StoreColOp<T>{1, 0, tot0.p, n}, sp, s);
      if (!lean) launch_reduce_cols<T, StoreColOp<T>>(part1.p, nparts, n_pad, StoreColOp<T>{1, 0, tot1.p, n}, sp, s);
    } else if (a.cols == POGS_AMD_PASS_COLS_PACK) {
      PackJobs pj;
      pj.j[0] = jd; pj.j[1] = js; pj.njobs = iter ? 2 : 0;
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
  } else if (exact) {
    launch_stream<T, true, true, false, kFull, Tag>(p, sa, ExactRowOp<T>{y12.p, yt.p, ycur.p, zs}, s);
    const SumJob jr{spart.p, grid, 1, S.p};
    launch_sum_jobs(&jr, 1, s);
    launch_reduce_cols<T, ExactColOp<T>>(part0.p, nparts, n_pad, ExactColOp<T>{x12.p, xt.p, x_cur.p, zs, n}, sp, s);
    const SumJob jc{sp, gridR, 1, S.p + 8};
    launch_sum_jobs(&jc, 1, s);
    launch_reduce_cols<T, StoreColOp<T>>(part0.p, nparts, n_pad, StoreColOp<T>{1, 0, tot0.p, n}, sp2, s);
  } else {
    sa.xin_add = x1.p;
    launch_stream<T, true, true, false, kLower, Tag>(p, sa, IdentRowOp<T>{}, s);
    launch_reduce_cols<T, StoreColOp<T>>(part0.p, nparts, n_pad, StoreColOp<T>{1, 0, tot0.p, n}, sp, s);
  }
  POGS_HIP_CHECK(hipGetLastError());
  POGS_HIP_CHECK(hipDeviceSynchronize());
  if (iter) { down(a.ytemp, ytemp); down(a.ynew, ynew); down(a.y12s, y12s); down(a.ytemps, ytemps); }
  down(a.dots, dots);
  down(a.tot0, tot0); down(a.tot1, tot1);
  if (pre || iter) { down(a.x12, x12); down(a.xtemp, xtemp); down(a.rhs, rhs); }
  if (a.pack) POGS_HIP_CHECK(hipMemcpy(a.pack, pack.p, pack_count * sizeof(double), hipMemcpyDeviceToHost));
  double Sh[16];
  POGS_HIP_CHECK(hipMemcpy(Sh, S.p, sizeof(Sh), hipMemcpyDeviceToHost));
  if (a.scalars) std::memcpy(a.scalars, Sh, 6 * sizeof(double));
  if (a.col_scalars) std::memcpy(a.col_scalars, Sh + 8, 4 * sizeof(double));
  const int out[8] = {p.tpb, p.nv, R, grid, stream_windows<T>(p, n_pad), kernel, nparts, p.xl ? 1 : 0};
  for (int i = 0; i < 8; ++i) a.info[i] = out[i];
}

}  // namespace pogs_amd

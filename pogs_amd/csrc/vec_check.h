#pragma once
// PogsAmdVecCheck (include/pogs_amd.h, Part 3): ONE launch of the element-wise kernels (vec_kernels.hip) on HOST arrays,
// and the scalar block's way to the host (engine.h: Ctx::queue_sum / fetch_scalars), through the launch functions and the
// block-count helpers the solvers call -- nothing here restates them.  vec_check_validate runs every refusal before any
// device work; vec_check_t runs the op.
#include <cstring>
#include <string>

#include "../../include/pogs_amd.h"
#include "common.h"
#include "engine.h"
#include "prox.h"
#include "vec_kernels.h"

namespace pogs_amd {

static_assert(kNumSlots <= POGS_AMD_VEC_SCALARS, "the header's scalar block holds the device's");

// arrays an op names: the first xin / xout / yin / yout entries must be given, the next *_opt may be
struct VecNeed {
  int xin, xout, yin, yout;
  int xout_opt, yout_opt;
  bool g, f, y_side;
};
inline VecNeed vec_need(int op) {
  switch (op) {
    case POGS_AMD_VEC_SCALE_OBJECTIVE: return {1, 4, 0, 0, 0, 0, true, false, false};
    case POGS_AMD_VEC_PROBE_UNIFORM: return {0, 0, 0, 0, 0, 0, true, false, false};
    case POGS_AMD_VEC_ADMM_PRE: return {2, 2, 2, 2, 1, 1, true, true, true};
    case POGS_AMD_VEC_ADMM_TAIL: return {3, 1, 0, 0, 0, 0, false, false, false};
    case POGS_AMD_VEC_UNSCALE: return {4, 1, 4, 2, 1, 0, false, false, true};
    case POGS_AMD_VEC_EXACT_U: return {3, 1, 0, 0, 0, 0, false, false, false};
    case POGS_AMD_VEC_SCALE_BY: return {2, 1, 0, 0, 0, 0, false, false, false};
    case POGS_AMD_VEC_AXPBY: return {1, 1, 0, 0, 0, 0, false, false, false};
    case POGS_AMD_VEC_SCAL: case POGS_AMD_VEC_SQRT: case POGS_AMD_VEC_FILL: return {0, 1, 0, 0, 0, 0, false, false, false};
    default: return {0, 0, 0, 0, 0, 0, false, false, false};
  }
}

inline void vec_refuse(bool ok, const std::string &msg) {
  if (!ok) throw Error(msg);
}

// the reach of one sum job inside `partials` and the scalar block
inline void vec_check_job(const int *j, const char *name, int k, size_t partials_len, int slots) {
  const std::string at = std::string(name) + "[" + std::to_string(k) + "]";
  vec_refuse(j[1] >= 1, at + ": nparts must be >= 1");
  vec_refuse(j[2] >= 1 && j[2] <= 8, at + ": ns must be in [1, 8]");
  vec_refuse(j[3] >= 0 && j[4] >= 0 && j[0] >= 0, at + ": first, stride and offset must be >= 0");
  const size_t stride = j[3] > 0 ? j[3] : j[2];
  const size_t reach = static_cast<size_t>(j[0]) + j[4] + static_cast<size_t>(j[1] - 1) * stride + j[2];
  vec_refuse(reach <= partials_len, at + ": the records reach beyond partials_len");
  vec_refuse(j[5] >= 0 && j[5] + j[2] <= slots, at + ": slot .. slot + ns leaves the scalar block");
}

inline bool vec_writes_partials(int op) { return op == POGS_AMD_VEC_ADMM_PRE || op == POGS_AMD_VEC_ADMM_TAIL; }
inline size_t vec_partials_needed(const PogsAmdVecArgs &a) {
  if (a.op == POGS_AMD_VEC_ADMM_PRE) return (static_cast<size_t>(pre_blocks(a.n_x)) + pre_blocks(a.n_y)) * 3;
  if (a.op == POGS_AMD_VEC_ADMM_TAIL) return static_cast<size_t>(vec_blocks(a.n_x)) * 2;
  return 0;
}

// every refusal, before any device work; the messages name the argument
inline void vec_check_validate(const PogsAmdVecArgs &a) {
  POGS_CHECK(a.dtype == POGS_AMD_F32 || a.dtype == POGS_AMD_F64, "unknown dtype");
  POGS_CHECK(a.op >= POGS_AMD_VEC_SCALE_OBJECTIVE && a.op <= POGS_AMD_VEC_PUBLISH, "unknown op");
  POGS_CHECK(a.info, "null argument: info");
  const VecNeed need = vec_need(a.op);
  const bool vectors = a.op <= POGS_AMD_VEC_FILL;
  if (vectors) {
    POGS_CHECK(a.n_x >= 1 && a.len_x >= static_cast<size_t>(a.n_x), "n_x must be >= 1 and len_x >= n_x");
    if (need.y_side) POGS_CHECK(a.n_y >= 1 && a.len_y >= static_cast<size_t>(a.n_y), "n_y must be >= 1 and len_y >= n_y");
  }
  for (int k = 0; k < need.xin; ++k) vec_refuse(a.x_in[k] != nullptr, "null argument: x_in[" + std::to_string(k) + "]");
  for (int k = 0; k < need.xout; ++k) vec_refuse(a.x_out[k] != nullptr, "null argument: x_out[" + std::to_string(k) + "]");
  for (int k = 0; k < need.yin; ++k) vec_refuse(a.y_in[k] != nullptr, "null argument: y_in[" + std::to_string(k) + "]");
  for (int k = 0; k < need.yout; ++k) vec_refuse(a.y_out[k] != nullptr, "null argument: y_out[" + std::to_string(k) + "]");
  if (need.g) POGS_CHECK(a.g_h && a.g_a && a.g_b && a.g_c && a.g_d && a.g_e, "null argument: g_h, g_a .. g_e");
  if (need.f) POGS_CHECK(a.f_h && a.f_a && a.f_b && a.f_c && a.f_d && a.f_e, "null argument: f_h, f_a .. f_e");
  switch (a.op) {
    case POGS_AMD_VEC_SCALE_OBJECTIVE: case POGS_AMD_VEC_SCALE_BY:
      POGS_CHECK(a.mode == 0 || a.mode == 1, "mode must be 0 (multiply) or 1 (divide)");
      break;
    case POGS_AMD_VEC_PROBE_UNIFORM:
      POGS_CHECK(a.scalars, "null argument: scalars");
      break;
    case POGS_AMD_VEC_ADMM_PRE: {
      POGS_CHECK(a.cheap == 0 || a.cheap == 1, "cheap must be 0 or 1");
      POGS_CHECK(a.probe == 0 || a.probe == 1, "probe must be 0 or 1");
      if (a.cheap) {
        bool all = true;
        for (int i = 0; i < a.n_x; ++i) all = all && is_cheap_prox(a.g_h[i]);
        for (int i = 0; i < a.n_y; ++i) all = all && is_cheap_prox(a.f_h[i]);
        POGS_CHECK(all, "cheap = 1 with a function outside is_cheap_prox");
      }
      if (!a.probe) POGS_CHECK((a.u_mask[0] & ~15) == 0 && (a.u_mask[1] & ~15) == 0, "u_mask must be in [0, 15]");
      POGS_CHECK(a.partials && a.scalars, "null argument: partials, scalars");
      POGS_CHECK(a.partials_len >= vec_partials_needed(a), "partials_len must hold [blocks_x + blocks_y][3]");
      break;
    }
    case POGS_AMD_VEC_ADMM_TAIL:
      POGS_CHECK(a.partials && a.scalars, "null argument: partials, scalars");
      POGS_CHECK(a.partials_len >= vec_partials_needed(a), "partials_len must hold [blocks][2]");
      break;
    case POGS_AMD_VEC_SUM_JOBS:
      POGS_CHECK(a.partials && a.scalars && a.jobs, "null argument: partials, scalars, jobs");
      POGS_CHECK(a.njobs >= 1 && a.njobs <= kMaxSumJobs, "njobs must be in [1, 8]");
      for (int k = 0; k < a.njobs; ++k) vec_check_job(a.jobs + 6 * k, "jobs", k, a.partials_len, POGS_AMD_VEC_SCALARS);
      break;
    case POGS_AMD_VEC_MAX_PARTIALS:
      POGS_CHECK(a.partials && a.scalars, "null argument: partials, scalars");
      POGS_CHECK(a.partials_len >= 1 && a.partials_len < (1u << 30), "partials_len must be in [1, 2^30)");
      break;
    case POGS_AMD_VEC_SUM_CG:
      POGS_CHECK(a.partials && a.scalars && a.jobs && a.cg, "null argument: partials, scalars, jobs, cg");
      POGS_CHECK(a.mode >= 1 && a.mode <= 3, "mode must be 1, 2 or 3");
      vec_check_job(a.jobs, "jobs", 0, a.partials_len, kNumSlots);
      break;
    case POGS_AMD_VEC_PUBLISH:
      POGS_CHECK(a.partials && a.scalars && a.pub, "null argument: partials, scalars, pub");
      POGS_CHECK(a.partials_len >= 1, "partials_len must be >= 1");
      POGS_CHECK(a.mode == 0 || a.mode == 1, "mode must be 0 (polling) or 1 (copying)");
      POGS_CHECK(a.njobs >= 0 && a.njobs <= kMaxSumJobs && (a.njobs == 0 || a.jobs), "njobs must be in [0, 8], with jobs");
      POGS_CHECK(a.njobs2 >= 0 && a.njobs2 <= kMaxSumJobs && (a.njobs2 == 0 || a.jobs2), "njobs2 must be in [0, 8], with jobs2");
      POGS_CHECK(a.njobs2 != a.njobs, "njobs2 must differ from njobs");
      for (int k = 0; k < a.njobs; ++k) vec_check_job(a.jobs + 6 * k, "jobs", k, a.partials_len, kNumSlots);
      for (int k = 0; k < a.njobs2; ++k) vec_check_job(a.jobs2 + 6 * k, "jobs2", k, a.partials_len, kNumSlots);
      for (int q = 0; q < 2; ++q)
        POGS_CHECK(a.ov_n[q] >= 0 && a.ov_slot[q] >= 0 && a.ov_slot[q] + a.ov_n[q] <= kNumSlots, "ov_slot, ov_n: the range leaves the scalar block");
      POGS_CHECK(a.ov_n[0] + a.ov_n[1] == 0 || a.ov_src, "null argument: ov_src");
      break;
    default: break;
  }
}

inline SumJob vec_sum_job(const int *j, const double *partials, double *S) {
  return SumJob{partials + j[0], j[1], j[2], S + j[5], j[3], j[4]};
}

// ops that need no arithmetic type: the scalar sums and the publish path
inline void vec_check_scalars(const PogsAmdVecArgs &a) {
  hipStream_t s = nullptr;
  DevBuf<double> part(a.partials_len);
  POGS_HIP_CHECK(hipMemcpy(part.p, a.partials, a.partials_len * sizeof(double), hipMemcpyHostToDevice));
  if (a.op == POGS_AMD_VEC_PUBLISH) {
    Ctx ctx;
    ctx.init(-1, 0);
    POGS_HIP_CHECK(hipMemcpyAsync(ctx.S.p, a.scalars, kNumSlots * sizeof(double), hipMemcpyHostToDevice, ctx.stream));
    POGS_HIP_CHECK(hipStreamSynchronize(ctx.stream));
    DevBuf<double> src(static_cast<size_t>(a.ov_n[0] + a.ov_n[1]) + 1);
    if (a.ov_n[0] + a.ov_n[1] > 0)
      POGS_HIP_CHECK(hipMemcpy(src.p, a.ov_src, static_cast<size_t>(a.ov_n[0] + a.ov_n[1]) * sizeof(double), hipMemcpyHostToDevice));
    if (a.mode == 1) ctx.poll_fetch = false;
    for (int round = 0; round < 2; ++round) {
      const int nj = round == 0 ? a.njobs : a.njobs2;
      const int *jobs = round == 0 ? a.jobs : a.jobs2;
      for (int k = 0; k < nj; ++k) ctx.queue_sum(vec_sum_job(jobs + 6 * k, part.p, ctx.S.p));
      if (round == 0) {
        ScalarOverlay ov;
        ov.src = src.p;
        ov.slot[0] = a.ov_slot[0]; ov.slot[1] = a.ov_slot[1];
        ov.n[0] = a.ov_n[0]; ov.n[1] = a.ov_n[1];
        ctx.set_overlay(ov);
      }
      const double *Sh = ctx.fetch_scalars();
      double *out = a.pub + static_cast<size_t>(round) * 2 * POGS_AMD_VEC_SCALARS;
      std::memcpy(out, Sh, kNumSlots * sizeof(double));
      POGS_HIP_CHECK(hipStreamSynchronize(ctx.stream));
      POGS_HIP_CHECK(hipMemcpy(out + POGS_AMD_VEC_SCALARS, ctx.S.p, kNumSlots * sizeof(double), hipMemcpyDeviceToHost));
      unsigned counter = 0;
      POGS_HIP_CHECK(hipMemcpy(&counter, ctx.pub_counter.p, sizeof(counter), hipMemcpyDeviceToHost));
      a.info[round] = static_cast<int>(counter);
      a.info[2 + round] = ctx.poll_fetch ? 1 : 0;
    }
    return;
  }
  DevBuf<double> S(POGS_AMD_VEC_SCALARS);
  POGS_HIP_CHECK(hipMemcpy(S.p, a.scalars, S.n * sizeof(double), hipMemcpyHostToDevice));
  DevBuf<double> cg(5);
  if (a.op == POGS_AMD_VEC_SUM_JOBS) {
    SumJob j[kMaxSumJobs];
    for (int k = 0; k < a.njobs; ++k) j[k] = vec_sum_job(a.jobs + 6 * k, part.p, S.p);
    launch_sum_jobs(j, a.njobs, s);
  } else if (a.op == POGS_AMD_VEC_MAX_PARTIALS) {
    launch_max_partials(part.p, static_cast<int>(a.partials_len), S.p, s);
  } else {
    POGS_HIP_CHECK(hipMemcpy(cg.p, a.cg, 5 * sizeof(double), hipMemcpyHostToDevice));
    launch_sum_cg(vec_sum_job(a.jobs, part.p, S.p), S.p, cg.p, a.mode, a.s0, a.s1, s);
  }
  POGS_HIP_CHECK(hipGetLastError());
  POGS_HIP_CHECK(hipDeviceSynchronize());
  POGS_HIP_CHECK(hipMemcpy(a.scalars, S.p, S.n * sizeof(double), hipMemcpyDeviceToHost));
  if (a.op == POGS_AMD_VEC_SUM_CG) POGS_HIP_CHECK(hipMemcpy(a.cg, cg.p, 5 * sizeof(double), hipMemcpyDeviceToHost));
}

template <typename T>
void vec_check_t(const PogsAmdVecArgs &a) {
  hipStream_t s = nullptr;
  const size_t lx = a.len_x, ly = a.len_y;
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
  const VecNeed need = vec_need(a.op);
  DevBuf<T> xi[4], xo[4], yi[4], yo[4];
  for (int k = 0; k < need.xin; ++k) up(xi[k], a.x_in[k], lx);
  for (int k = 0; k < need.xout + need.xout_opt; ++k) up(xo[k], a.x_out[k], lx);
  for (int k = 0; k < need.yin; ++k) up(yi[k], a.y_in[k], ly);
  for (int k = 0; k < need.yout + need.yout_opt; ++k) up(yo[k], a.y_out[k], ly);
  FnBuf<T> g, f;
  if (need.g) up_fn(g, a.g_h, a.g_a, a.g_b, a.g_c, a.g_d, a.g_e, lx);
  if (need.f) up_fn(f, a.f_h, a.f_a, a.f_b, a.f_c, a.f_d, a.f_e, ly);
  // partial sums start as NaN: a slot no workgroup wrote shows in every total that reads it
  DevBuf<double> part, S, cg;
  if (vec_writes_partials(a.op)) {
    part.alloc(a.partials_len);
    POGS_HIP_CHECK(hipMemset(part.p, 0xFF, a.partials_len * sizeof(double)));
    S.alloc(POGS_AMD_VEC_SCALARS);
    POGS_HIP_CHECK(hipMemcpy(S.p, a.scalars, S.n * sizeof(double), hipMemcpyHostToDevice));
  }
  const T rho = static_cast<T>(a.rho), alpha = static_cast<T>(a.alpha), zs = static_cast<T>(a.zs);
  const T s0 = static_cast<T>(a.s0), s1 = static_cast<T>(a.s1);
  const int n = a.n_x;
  switch (a.op) {
    case POGS_AMD_VEC_SCALE_OBJECTIVE:
      launch_scale_objective<T>(g.view(), xo[0].p, xo[1].p, xo[2].p, xo[3].p, xi[0].p, n, a.mode == 1, s);
      break;
    case POGS_AMD_VEC_PROBE_UNIFORM: {
      const FnUniform<T> u = probe_uniform<T>(g.view(), n, s);
      a.info[0] = u.mask; a.info[1] = u.h;
      a.scalars[0] = static_cast<double>(u.c); a.scalars[1] = static_cast<double>(u.d); a.scalars[2] = static_cast<double>(u.e);
      break;
    }
    case POGS_AMD_VEC_ADMM_PRE: {
      AdmmPreArgs<T> pa;
      pa.n_x = a.n_x; pa.n_y = a.n_y;
      pa.g = g.view(); pa.f = f.view();
      pa.x_cur = xi[0].p; pa.xt = xi[1].p; pa.y_cur = yi[0].p; pa.yt = yi[1].p;
      pa.zt_scale = zs;
      pa.x12 = xo[0].p; pa.xtemp = xo[1].p; pa.y12 = yo[0].p; pa.ytemp = yo[1].p;
      pa.rho = rho; pa.alpha = alpha; pa.cheap = a.cheap == 1;
      pa.partials = part.p;
      pa.blocks_x = pre_blocks(a.n_x);
      pa.x_aux = xo[2].p; pa.y_aux = yo[2].p;
      if (a.cg) {
        cg.alloc(2);
        POGS_HIP_CHECK(hipMemcpy(cg.p, a.cg, 2 * sizeof(double), hipMemcpyHostToDevice));
        pa.cg_reset = cg.p;
      }
      if (a.probe) {
        pa.ug = probe_uniform<T>(pa.g, a.n_x, s);
        pa.uf = probe_uniform<T>(pa.f, a.n_y, s);
      } else {
        FnUniform<T> *u[2] = {&pa.ug, &pa.uf};
        for (int q = 0; q < 2; ++q) {
          u[q]->mask = a.u_mask[q]; u[q]->h = a.u_h[q];
          u[q]->c = static_cast<T>(a.u_cde[3 * q]); u[q]->d = static_cast<T>(a.u_cde[3 * q + 1]); u[q]->e = static_cast<T>(a.u_cde[3 * q + 2]);
        }
      }
      launch_admm_pre<T>(pa, s);
      // the two jobs of the dense iteration (dense_iter.h: iteration, step 1)
      SumJob j[2] = {{part.p, pa.blocks_x, 3, S.p + kGapX},
                     {part.p + static_cast<size_t>(pa.blocks_x) * 3, pre_blocks(a.n_y), 3, S.p + kGapY}};
      launch_sum_jobs(j, 2, s);
      a.info[0] = pa.blocks_x; a.info[1] = pre_blocks(a.n_y); a.info[2] = pa.ug.mask; a.info[3] = pa.uf.mask;
      break;
    }
    case POGS_AMD_VEC_ADMM_TAIL: {
      launch_admm_tail<T>(n, xi[0].p, xi[1].p, xi[2].p, xo[0].p, part.p, s);
      const SumJob j{part.p, vec_blocks(n), 2, S.p + kDXprev2};
      launch_sum_jobs(&j, 1, s);
      a.info[0] = vec_blocks(n);
      break;
    }
    case POGS_AMD_VEC_UNSCALE: {
      UnscaleArgs<T> ua;
      ua.n_x = a.n_x; ua.n_y = a.n_y;
      ua.x12 = xi[0].p; ua.xt = xi[1].p; ua.xprev = xi[2].p; ua.e = xi[3].p;
      ua.y12 = yi[0].p; ua.yt = yi[1].p; ua.yprev = yi[2].p; ua.d = yi[3].p;
      ua.zt_scale = zs; ua.rho = rho;
      ua.x_out = xo[0].p; ua.mu_out = xo[1].p; ua.y_out = yo[0].p; ua.l_out = yo[1].p;
      launch_unscale<T>(ua, s);
      break;
    }
    case POGS_AMD_VEC_EXACT_U: launch_exact_u<T>(n, xi[0].p, xi[1].p, xi[2].p, s0, xo[0].p, s); break;
    case POGS_AMD_VEC_SCALE_BY: launch_scale_by<T>(n, s0, xi[0].p, xi[1].p, a.mode == 1, xo[0].p, s); break;
    case POGS_AMD_VEC_AXPBY: launch_axpby<T>(n, s0, xi[0].p, s1, xo[0].p, s); break;
    case POGS_AMD_VEC_SCAL: launch_scal<T>(xo[0].p, s0, n, s); break;
    case POGS_AMD_VEC_SQRT: launch_sqrt_inplace<T>(xo[0].p, n, s); break;
    case POGS_AMD_VEC_FILL: launch_fill<T>(xo[0].p, s0, n, s); break;
    default: throw Error("unknown op");
  }
  POGS_HIP_CHECK(hipGetLastError());
  POGS_HIP_CHECK(hipDeviceSynchronize());
  for (int k = 0; k < 4; ++k) { down(a.x_out[k], xo[k]); down(a.y_out[k], yo[k]); }
  if (vec_writes_partials(a.op)) {
    POGS_HIP_CHECK(hipMemcpy(a.partials, part.p, a.partials_len * sizeof(double), hipMemcpyDeviceToHost));
    POGS_HIP_CHECK(hipMemcpy(a.scalars, S.p, S.n * sizeof(double), hipMemcpyDeviceToHost));
  }
  if (cg.p) POGS_HIP_CHECK(hipMemcpy(a.cg, cg.p, 2 * sizeof(double), hipMemcpyDeviceToHost));
}

// PogsAmdVecCheck: refusals first (no device), then the op
inline void vec_check(const PogsAmdVecArgs *a) {
  POGS_CHECK(a != nullptr, "null argument: args");
  vec_check_validate(*a);
  if (a->op >= POGS_AMD_VEC_SUM_JOBS) return vec_check_scalars(*a);
  if (a->dtype == POGS_AMD_F32) vec_check_t<float>(*a);
  else vec_check_t<double>(*a);
}

}  // namespace pogs_amd

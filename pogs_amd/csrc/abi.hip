// extern "C" entry points (include/pogs_amd.h).  No exception crosses this file.
#include <cmath>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "engine.h"
#include "factor_check.h"
#include "many_kernels.h"
#include "pass_check.h"
#include "pass_check_mixed.h"
#include "sparse_batch_kernels.h"
#include "sparse_direct.h"
#include "spmv_check.h"
#include "prox.h"
#include "stream.h"
#include "stream_mixed_check.h"
#include "vec_check.h"
#include "vec_kernels.h"

namespace pogs_amd {

static_assert(kTriLower == kLower && kTriUpper == kUpper, "sparse_direct.h restates stream.h's Tri");

// One factory per streaming shape and arithmetic type (dense_plan.hip, built once per entry of
// POGS_STREAM_PLANS plus the windowed form): the shape follows from the stored row length alone,
// so it is chosen here and only that translation unit's code object is ever loaded.
#define POGS_DECLARE_PLAN(TPB_, NV_)                                                                               \
  SolverBase *make_dense_solver_f32_p##TPB_##_##NV_(int, size_t, size_t, const void *, int, const PogsAmdOptions *, \
                                                    const PogsAmdDist *);                                          \
  SolverBase *make_dense_solver_f64_p##TPB_##_##NV_(int, size_t, size_t, const void *, int, const PogsAmdOptions *, \
                                                    const PogsAmdDist *);                                          \
  void dense_pass_check_f32_p##TPB_##_##NV_(const PogsAmdDensePassArgs *, int);                                    \
  void dense_pass_check_f64_p##TPB_##_##NV_(const PogsAmdDensePassArgs *, int);
POGS_STREAM_PLANS(POGS_DECLARE_PLAN)
#undef POGS_DECLARE_PLAN
SolverBase *make_dense_solver_f32_xl(int, size_t, size_t, const void *, int, const PogsAmdOptions *, const PogsAmdDist *);
SolverBase *make_dense_solver_f64_xl(int, size_t, size_t, const void *, int, const PogsAmdOptions *, const PogsAmdDist *);
void dense_pass_check_f32_xl(const PogsAmdDensePassArgs *, int);
void dense_pass_check_f64_xl(const PogsAmdDensePassArgs *, int);

template <typename T>
inline StreamPlan dense_plan_for(size_t m, size_t n, const PogsAmdOptions *opt, const PogsAmdDist *dist) {
  // the stored row length, as DenseSolver's constructor derives it
  const size_t m_global = (dist && dist->world >= 1) ? dist->m_global : m;
  const bool tall = m_global > n;
  const bool cgls = opt && (opt->projector == POGS_AMD_PROJ_CGLS || opt->projector == POGS_AMD_PROJ_CGLS_FUSED);
  const size_t stored_cols = (!tall && !cgls) ? m : n;
  return make_stream_plan<T>(static_cast<int>(round_up(stored_cols, Vec16<T>::N)), 256);
}

inline SolverBase *make_dense_solver(int dtype, int ord, size_t m, size_t n, const void *A, int mem,
                                     const PogsAmdOptions *opt, const PogsAmdDist *dist) {
  POGS_CHECK(dtype == POGS_AMD_F32 || dtype == POGS_AMD_F64, "unknown dtype");
  POGS_CHECK(m > 0 && n > 0 && m < (1u << 31) && n < (1u << 31), "bad dimensions");
  const bool f32 = dtype == POGS_AMD_F32;
  const StreamPlan p = f32 ? dense_plan_for<float>(m, n, opt, dist) : dense_plan_for<double>(m, n, opt, dist);
  POGS_CHECK(p.ok, "no streaming shape for this matrix");
  if (p.xl) return f32 ? make_dense_solver_f32_xl(ord, m, n, A, mem, opt, dist) : make_dense_solver_f64_xl(ord, m, n, A, mem, opt, dist);
#define POGS_PICK_PLAN(TPB_, NV_)                                                          \
  if (p.tpb == TPB_ && p.nv == NV_)                                                        \
    return f32 ? make_dense_solver_f32_p##TPB_##_##NV_(ord, m, n, A, mem, opt, dist)       \
               : make_dense_solver_f64_p##TPB_##_##NV_(ord, m, n, A, mem, opt, dist);
  POGS_STREAM_PLANS(POGS_PICK_PLAN)
#undef POGS_PICK_PLAN
  throw Error("no dense solver for this streaming shape");
}

// PogsAmdDensePassCheck: refusals first (no device), then the object of the shape, as make_dense_solver picks it
inline void dense_pass_check(const PogsAmdDensePassArgs *a) {
  POGS_CHECK(a != nullptr, "null argument: args");
  pass_check_validate(*a);
  int num_cu = a->num_cu;
  if (num_cu == 0) {
    int dev = 0;
    hipDeviceProp_t prop;
    POGS_HIP_CHECK(hipGetDevice(&dev));
    POGS_HIP_CHECK(hipGetDeviceProperties(&prop, dev));
    num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  }
  const bool f32 = a->dtype == POGS_AMD_F32;
  const StreamPlan p = f32 ? pass_check_plan<float>(*a, num_cu) : pass_check_plan<double>(*a, num_cu);
  if (p.xl) return f32 ? dense_pass_check_f32_xl(a, num_cu) : dense_pass_check_f64_xl(a, num_cu);
#define POGS_PICK_PLAN(TPB_, NV_)                                                          \
  if (p.tpb == TPB_ && p.nv == NV_)                                                        \
    return f32 ? dense_pass_check_f32_p##TPB_##_##NV_(a, num_cu) : dense_pass_check_f64_p##TPB_##_##NV_(a, num_cu);
  POGS_STREAM_PLANS(POGS_PICK_PLAN)
#undef POGS_PICK_PLAN
  throw Error("no dense pass check for this streaming shape");
}
// The storage option (PogsAmdOptStorage) of PogsAmdCreateDense: every combination POGS_AMD_STORE_F32 is not honoured
// for is refused here, before anything is built (include/pogs_amd.h)
inline void check_dense_storage(int dtype, size_t m, size_t n, const PogsAmdOptions *opt, const PogsAmdDist *dist) {
  if (!opt || PogsAmdOptStorage(opt) == POGS_AMD_STORE_SAME) return;
  POGS_CHECK(PogsAmdOptStorage(opt) == POGS_AMD_STORE_F32, "storage: unknown value (POGS_AMD_STORE_SAME or POGS_AMD_STORE_F32)");
  POGS_CHECK(dtype == POGS_AMD_F64, "storage POGS_AMD_STORE_F32 needs dtype POGS_AMD_F64 (an fp32 handle already stores floats)");
  POGS_CHECK(!(dist && dist->world >= 1), "storage POGS_AMD_STORE_F32 is single-GPU (row shards are not supported)");
  POGS_CHECK(m > n, "storage POGS_AMD_STORE_F32 needs m > n");
  POGS_CHECK(opt->projector == POGS_AMD_PROJ_DEFAULT || opt->projector == POGS_AMD_PROJ_DIRECT,
             "storage POGS_AMD_STORE_F32 needs the direct projector (not CGLS or CGLS_FUSED)");
  POGS_CHECK(n < (1u << 31) && make_mixed_plan(n, 256).ok,
             "storage POGS_AMD_STORE_F32: the row is too wide (windowed, or past the 10240 columns the one-pass iteration reaches)");
}

// PogsAmdDensePassMixedCheck: refusals first (no device), then the launches (pass_check_mixed.h)
inline void dense_pass_mixed_check(const PogsAmdDensePassArgs *a) {
  POGS_CHECK(a != nullptr, "null argument: args");
  pass_mixed_check_validate(*a);
  int num_cu = a->num_cu;
  if (num_cu == 0) {
    int dev = 0;
    hipDeviceProp_t prop;
    POGS_HIP_CHECK(hipGetDevice(&dev));
    POGS_HIP_CHECK(hipGetDeviceProperties(&prop, dev));
    num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  }
  pass_mixed_check_run(*a, num_cu);
}

// PogsAmdStreamMixedCheck: refusals first (no device), then the launches (stream_mixed_check.h)
inline void stream_mixed_check(const StreamMixedCheckArgs &a) {
  stream_mixed_check_validate(a);
  int num_cu = a.num_cu;
  if (num_cu == 0) {
    int dev = 0;
    hipDeviceProp_t prop;
    POGS_HIP_CHECK(hipGetDevice(&dev));
    POGS_HIP_CHECK(hipGetDeviceProperties(&prop, dev));
    num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  }
  stream_mixed_check_run(a, num_cu);
}

SolverBase *make_sparse_solver(int dtype, int ord, size_t m, size_t n, size_t nnz, const void *data,
                               const int *ptr, const int *ind, int mem, const PogsAmdOptions *opt,
                               const PogsAmdDist *dist);
SolverBase *make_sparse_solver_mixed(int ord, size_t m, size_t n, size_t nnz, const double *data, const int *ptr,
                                     const int *ind, int mem, const PogsAmdOptions *opt);

// gsl::rand (src/cpu/include/gsl/gsl_rand.h:8-16): a fresh
// std::default_random_engine (libstdc++: minstd_rand0, x <- 16807 x mod 2^31-1,
// seed 1) feeding uniform_real_distribution<T>(0,1) = generate_canonical: one
// draw per float, two per double.  Restated so the Norm2Est start vector does
// not depend on the C++ standard library in use.
namespace {
struct MinStd0 {
  uint64_t s = 1;
  uint32_t next() {
    s = (s * 16807ull) % 2147483647ull;
    return static_cast<uint32_t>(s);
  }
};
}  // namespace
void rand_uniform_host(float *x, size_t n) {
  MinStd0 g;
  const float r = static_cast<float>(2147483646.0L);
  for (size_t i = 0; i < n; ++i) {
    float v = static_cast<float>(g.next() - 1u) / r;
    if (v >= 1.0f) v = std::nextafter(1.0f, 0.0f);
    x[i] = v;
  }
}
void rand_uniform_host(double *x, size_t n) {
  MinStd0 g;
  const double r = 2147483646.0;
  for (size_t i = 0; i < n; ++i) {
    const double lo = static_cast<double>(g.next() - 1u);
    const double hi = static_cast<double>(g.next() - 1u);
    double v = (lo + hi * r) / (r * r);
    if (v >= 1.0) v = std::nextafter(1.0, 0.0);
    x[i] = v;
  }
}

namespace {

thread_local std::string g_last_error;

// `h` (may be null): the handle the entry point works on.  An error inside a row-sharded solve
// aborts the handle's communicator (SolverBase::on_error), so that the peers' next collective
// fails or times out instead of waiting for this rank for ever.
template <typename F>
int guarded(F &&fn, PogsAmdSolver *h = nullptr) {
  auto failed = [&](const char *what) {
    g_last_error = what;
    std::fprintf(stderr, "pogs_amd: %s\n", what);
    try {
      if (h && h->impl) h->impl->on_error();
    } catch (...) {}
    return POGS_ERROR;
  };
  try {
    g_last_error.clear();
    if (h && h->impl) h->impl->on_entry();
    return fn();
  } catch (const std::exception &e) {
    return failed(e.what());
  } catch (...) {
    return failed("unknown error");
  }
}

SolveParams make_params(double rho, double abs_tol, double rel_tol, unsigned max_iter, unsigned verbose,
                        int adaptive_rho, int gap_stop) {
  SolveParams p;
  p.rho = rho; p.abs_tol = abs_tol; p.rel_tol = rel_tol;
  p.max_iter = max_iter == 0 ? 1 : max_iter;
  p.verbose = verbose;
  p.adaptive_rho = adaptive_rho != 0;
  p.gap_stop = gap_stop != 0;
  return p;
}

// The array entry points (the reference's four and PogsAmdSolve / PogsAmdBeginRun) take TWELVE arrays: a null one is a
// caller's mistake there, not a broadcast field (that reading belongs to the *Fn entry points alone) -- without the
// check the solve would run on the defaults (a = c = 1, b = d = e = 0, h = kZero) and return a plausible wrong answer.
FnHost fn_arrays(const void *a, const void *b, const void *c, const void *d, const void *e, const int *h, const char *which) {
  if (!(a && b && c && d && e && h))
    throw Error(std::string("null coefficient array in the description of ") + which +
                " (a, b, c, d, e, h must all be given; broadcast fields: PogsAmdSolveFn)");
  return FnHost{a, b, c, d, e, h};
}

// One-shot dense solve: src/interface_c/pogs_c.cpp:9-55.
template <typename T>
int pogs_dense(enum ORD ord, size_t m, size_t n, const T *A, const T *f_a, const T *f_b, const T *f_c,
               const T *f_d, const T *f_e, const enum FUNCTION *f_h, const T *g_a, const T *g_b, const T *g_c,
               const T *g_d, const T *g_e, const enum FUNCTION *g_h, T rho, T abs_tol, T rel_tol,
               unsigned max_iter, unsigned verbose, int adaptive_rho, int gap_stop, T *x, T *y, T *l, T *optval,
               unsigned *final_iter) {
  return guarded([&]() {
    const FnHost f = fn_arrays(f_a, f_b, f_c, f_d, f_e, reinterpret_cast<const int *>(f_h), "f");
    const FnHost g = fn_arrays(g_a, g_b, g_c, g_d, g_e, reinterpret_cast<const int *>(g_h), "g");
    std::unique_ptr<SolverBase> s(make_dense_solver(sizeof(T) == 4 ? POGS_AMD_F32 : POGS_AMD_F64, ord, m, n, A,
                                                    POGS_AMD_HOST, nullptr, nullptr));
    double ov = 0;
    const int st = s->solve(f, g, make_params(rho, abs_tol, rel_tol, max_iter, verbose, adaptive_rho, gap_stop),
                            x, y, l, nullptr, &ov, final_iter);
    *optval = static_cast<T>(ov);
    return st;
  });
}

// One-shot sparse solve: src/interface_c/pogs_c.cpp:57-108.
template <typename T>
int pogs_sparse(enum ORD ord, size_t m, size_t n, size_t nnz, const T *data, const int *ptr, const int *ind,
                const T *f_a, const T *f_b, const T *f_c, const T *f_d, const T *f_e, const enum FUNCTION *f_h,
                const T *g_a, const T *g_b, const T *g_c, const T *g_d, const T *g_e, const enum FUNCTION *g_h,
                T rho, T abs_tol, T rel_tol, unsigned max_iter, unsigned verbose, int adaptive_rho, int gap_stop,
                T *x, T *y, T *l, T *optval, unsigned *final_iter) {
  return guarded([&]() {
    const FnHost f = fn_arrays(f_a, f_b, f_c, f_d, f_e, reinterpret_cast<const int *>(f_h), "f");
    const FnHost g = fn_arrays(g_a, g_b, g_c, g_d, g_e, reinterpret_cast<const int *>(g_h), "g");
    std::unique_ptr<SolverBase> s(make_sparse_solver(sizeof(T) == 4 ? POGS_AMD_F32 : POGS_AMD_F64, ord, m, n, nnz,
                                                     data, ptr, ind, POGS_AMD_HOST, nullptr, nullptr));
    double ov = 0;
    const int st = s->solve(f, g, make_params(rho, abs_tol, rel_tol, max_iter, verbose, adaptive_rho, gap_stop),
                            x, y, l, nullptr, &ov, final_iter);
    *optval = static_cast<T>(ov);
    return st;
  });
}

template <typename T>
void prox_eval_host(size_t n, const int *h, const void *a, const void *b, const void *c, const void *d,
                    const void *e, double rho, const void *in, void *out, double *fsum, const void *xin = nullptr) {
  POGS_CHECK(n < (1u << 31), "n too large");
  hipStream_t s = nullptr;
  const int cnt = static_cast<int>(n);
  FnBuf<T> fb;
  fb.alloc(n);
  DevBuf<T> vin(n), vout(n);
  auto up = [&](void *dst, const void *src, size_t bytes) {
    POGS_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s));
  };
  up(fb.h.p, h, n * sizeof(int));
  up(fb.a.p, a, n * sizeof(T)); up(fb.b.p, b, n * sizeof(T)); up(fb.c.p, c, n * sizeof(T));
  up(fb.d.p, d, n * sizeof(T)); up(fb.e.p, e, n * sizeof(T));
  up(vin.p, in, n * sizeof(T));
  {
    FnHost fh{a, b, c, d, e, h};
    warn_negative_coeffs<T>(fh, n);
  }
  // clamp c, e >= 0 as FunctionObj's constructor does (prox_lib.h:62-69): scale by 1.
  DevBuf<T> ones(n);
  launch_fill<T>(ones.p, static_cast<T>(1), n, s);
  launch_scale_objective<T>(fb.view(), fb.a.p, fb.c.p, fb.d.p, fb.e.p, ones.p, cnt, false, s);
  if (out && xin) {   // ProjSubgradEval: `in` is v, `xin` the point x
    DevBuf<T> xv(n);
    up(xv.p, xin, n * sizeof(T));
    launch_proj_subgrad<T>(cnt, fb.view(), xv.p, vin.p, vout.p, s);
    POGS_HIP_CHECK(hipMemcpyAsync(out, vout.p, n * sizeof(T), hipMemcpyDeviceToHost, s));
    POGS_HIP_CHECK(hipStreamSynchronize(s));   // xv is freed at scope exit
  } else if (out) {
    launch_prox_eval<T>(cnt, fb.view(), static_cast<T>(rho), vin.p, vout.p, s);
    POGS_HIP_CHECK(hipMemcpyAsync(out, vout.p, n * sizeof(T), hipMemcpyDeviceToHost, s));
  }
  if (fsum) {
    const int blocks = vec_blocks(cnt);
    DevBuf<double> part(blocks), tot(1);
    launch_func_eval<T>(cnt, fb.view(), vin.p, part.p, s);
    SumJob j{part.p, blocks, 1, tot.p};
    launch_sum_jobs(&j, 1, s);
    POGS_HIP_CHECK(hipMemcpyAsync(fsum, tot.p, sizeof(double), hipMemcpyDeviceToHost, s));
    POGS_HIP_CHECK(hipStreamSynchronize(s));
  }
  POGS_HIP_CHECK(hipStreamSynchronize(s));
}

// the one-pass kernels' logical workgroup id of every block of a launch (PogsAmdBlockIdCheck)
__global__ void __launch_bounds__(64) block_id_check_kernel(int *ids) {
  if (threadIdx.x == 0) ids[blockIdx.x] = dev::logical_block_id();
}

}  // namespace
}  // namespace pogs_amd

using namespace pogs_amd;

struct PogsAmdMany {
  std::unique_ptr<ManyHandle> impl;
};

namespace {
// What every create entry ends with: a new handle around the implementation `make()` builds, handed to *out only once
// that exists (a throw on the way leaves *out NULL and nothing behind).
template <typename Handle, typename Make>
void new_handle(Handle **out, Make make) {
  std::unique_ptr<Handle> h(new Handle);
  h->impl.reset(make());
  *out = h.release();
}

// What every many-problem entry refuses first: an empty call, then any projector but the direct one (`what`: the
// prefix of the two messages).
void check_many_call(const std::string &what, int k, const PogsAmdOptions *opt) {
  POGS_CHECK(k >= 1, (what + ": k must be >= 1").c_str());
  const int projector = opt ? opt->projector : POGS_AMD_PROJ_DEFAULT;
  POGS_CHECK(projector == POGS_AMD_PROJ_DEFAULT || projector == POGS_AMD_PROJ_DIRECT,
             (what + ": only the direct projector is supported (CGLS refused)").c_str());
}
}  // namespace

extern "C" {

int PogsD(enum ORD ord, size_t m, size_t n, const double *A, const double *f_a, const double *f_b,
          const double *f_c, const double *f_d, const double *f_e, const enum FUNCTION *f_h, const double *g_a,
          const double *g_b, const double *g_c, const double *g_d, const double *g_e, const enum FUNCTION *g_h,
          double rho, double abs_tol, double rel_tol, unsigned int max_iter, unsigned int verbose,
          int adaptive_rho, int gap_stop, double *x, double *y, double *l, double *optval,
          unsigned int *final_iter) {
  return pogs_dense<double>(ord, m, n, A, f_a, f_b, f_c, f_d, f_e, f_h, g_a, g_b, g_c, g_d, g_e, g_h, rho, abs_tol,
                            rel_tol, max_iter, verbose, adaptive_rho, gap_stop, x, y, l, optval, final_iter);
}

int PogsS(enum ORD ord, size_t m, size_t n, const float *A, const float *f_a, const float *f_b, const float *f_c,
          const float *f_d, const float *f_e, const enum FUNCTION *f_h, const float *g_a, const float *g_b,
          const float *g_c, const float *g_d, const float *g_e, const enum FUNCTION *g_h, float rho, float abs_tol,
          float rel_tol, unsigned int max_iter, unsigned int verbose, int adaptive_rho, int gap_stop, float *x,
          float *y, float *l, float *optval, unsigned int *final_iter) {
  return pogs_dense<float>(ord, m, n, A, f_a, f_b, f_c, f_d, f_e, f_h, g_a, g_b, g_c, g_d, g_e, g_h, rho, abs_tol,
                           rel_tol, max_iter, verbose, adaptive_rho, gap_stop, x, y, l, optval, final_iter);
}

int PogsSparseD(enum ORD ord, size_t m, size_t n, size_t nnz, const double *data, const int *ptr, const int *ind,
                const double *f_a, const double *f_b, const double *f_c, const double *f_d, const double *f_e,
                const enum FUNCTION *f_h, const double *g_a, const double *g_b, const double *g_c,
                const double *g_d, const double *g_e, const enum FUNCTION *g_h, double rho, double abs_tol,
                double rel_tol, unsigned int max_iter, unsigned int verbose, int adaptive_rho, int gap_stop,
                double *x, double *y, double *l, double *optval, unsigned int *final_iter) {
  return pogs_sparse<double>(ord, m, n, nnz, data, ptr, ind, f_a, f_b, f_c, f_d, f_e, f_h, g_a, g_b, g_c, g_d, g_e,
                             g_h, rho, abs_tol, rel_tol, max_iter, verbose, adaptive_rho, gap_stop, x, y, l, optval,
                             final_iter);
}

int PogsSparseS(enum ORD ord, size_t m, size_t n, size_t nnz, const float *data, const int *ptr, const int *ind,
                const float *f_a, const float *f_b, const float *f_c, const float *f_d, const float *f_e,
                const enum FUNCTION *f_h, const float *g_a, const float *g_b, const float *g_c, const float *g_d,
                const float *g_e, const enum FUNCTION *g_h, float rho, float abs_tol, float rel_tol,
                unsigned int max_iter, unsigned int verbose, int adaptive_rho, int gap_stop, float *x, float *y,
                float *l, float *optval, unsigned int *final_iter) {
  return pogs_sparse<float>(ord, m, n, nnz, data, ptr, ind, f_a, f_b, f_c, f_d, f_e, f_h, g_a, g_b, g_c, g_d, g_e,
                            g_h, rho, abs_tol, rel_tol, max_iter, verbose, adaptive_rho, gap_stop, x, y, l, optval,
                            final_iter);
}

int PogsAmdDistUniqueId(char *out) {
  return guarded([&]() {
    DistComm::unique_id(out);
    return 0;
  });
}

int PogsAmdCreateDense(PogsAmdSolver **out, int dtype, enum ORD ord, size_t m, size_t n, const void *A, int mem,
                       const PogsAmdOptions *opt, const PogsAmdDist *dist) {
  return guarded([&]() {
    *out = nullptr;
    check_dense_storage(dtype, m, n, opt, dist);   // refused before anything is built
    DeviceGuard guard(opt ? opt->device : -1);   // the caller's current device is put back on exit
    new_handle(out, [&] { return make_dense_solver(dtype, ord, m, n, A, mem, opt, dist); });
    return 0;
  });
}

int PogsAmdCreateSparse(PogsAmdSolver **out, int dtype, enum ORD ord, size_t m, size_t n, size_t nnz,
                        const void *data, const int *ptr, const int *ind, int mem, const PogsAmdOptions *opt,
                        const PogsAmdDist *dist) {
  return guarded([&]() {
    *out = nullptr;
    // refused before anything is built: the sparse CGLS loop already is device-resident with one pass per product
    POGS_CHECK(!(opt && opt->projector == POGS_AMD_PROJ_CGLS_FUSED),
               "POGS_AMD_PROJ_CGLS_FUSED is a dense projector (a sparse handle: POGS_AMD_PROJ_CGLS runs the device-resident loop)");
    POGS_CHECK(!(opt && PogsAmdOptStorage(opt) != POGS_AMD_STORE_SAME), "storage: a sparse handle stores its matrix in its dtype (POGS_AMD_STORE_SAME)");
    DeviceGuard guard(opt ? opt->device : -1);
    new_handle(out, [&] { return make_sparse_solver(dtype, ord, m, n, nnz, data, ptr, ind, mem, opt, dist); });
    return 0;
  });
}

int PogsAmdCreateSparseMixed(PogsAmdSolver **out, enum ORD ord, size_t m, size_t n, size_t nnz, const double *data,
                             const int *ptr, const int *ind, int mem, const PogsAmdOptions *opt) {
  return guarded([&]() {
    POGS_CHECK(out != nullptr, "null argument: out");
    *out = nullptr;
    // every refusal comes before anything is built (and before the first HIP call)
    POGS_CHECK(data && ptr && ind, "null argument: data, ptr and ind are required");
    POGS_CHECK(ord == ROW_MAJ || ord == COL_MAJ, "unknown ord (ROW_MAJ: CSR, COL_MAJ: CSC)");
    POGS_CHECK(mem == POGS_AMD_HOST || mem == POGS_AMD_DEVICE, "unknown mem (POGS_AMD_HOST or POGS_AMD_DEVICE)");
    POGS_CHECK(m > 0 && n > 0 && m < (1u << 31) && n < (1u << 31) && nnz < (1ull << 31), "bad dimensions");
    if (opt) {
      POGS_CHECK(opt->projector != POGS_AMD_PROJ_CGLS_FUSED,
                 "POGS_AMD_PROJ_CGLS_FUSED is a dense projector (a sparse handle: POGS_AMD_PROJ_CGLS runs the device-resident loop)");
      POGS_CHECK(opt->projector != POGS_AMD_PROJ_DIRECT || std::min(m, n) <= static_cast<size_t>(POGS_AMD_SPARSE_DIRECT_MAX),
                 "the sparse direct projector needs min(m, n) <= POGS_AMD_SPARSE_DIRECT_MAX; use POGS_AMD_PROJ_CGLS");
      POGS_CHECK(PogsAmdOptStorage(opt) == POGS_AMD_STORE_SAME || PogsAmdOptStorage(opt) == POGS_AMD_STORE_F32,
                 "storage: unknown value (a mixed sparse handle takes 0 or POGS_AMD_STORE_F32; it stores float non-zeros either way)");
    }
    DeviceGuard guard(opt ? opt->device : -1);
    new_handle(out,
               [&] { return make_sparse_solver_mixed(static_cast<int>(ord), m, n, nnz, data, ptr, ind, mem, opt); });
    return 0;
  });
}

int PogsAmdCreateDenseMixed(PogsAmdSolver **out, enum ORD ord, size_t m, size_t n, const double *A, int mem,
                            const PogsAmdOptions *opt) {
  return guarded([&]() {
    POGS_CHECK(out != nullptr, "null argument: out");
    *out = nullptr;
    // every refusal comes before anything is built (and before the first HIP call)
    POGS_CHECK(A && opt, "null argument: A and opt are required (opt->projector names POGS_AMD_PROJ_CGLS_FUSED)");
    POGS_CHECK(ord == ROW_MAJ || ord == COL_MAJ, "unknown ord (ROW_MAJ or COL_MAJ)");
    POGS_CHECK(mem == POGS_AMD_HOST || mem == POGS_AMD_DEVICE, "unknown mem (POGS_AMD_HOST or POGS_AMD_DEVICE)");
    POGS_CHECK(m > 0 && n > 0 && m < (1u << 31) && n < (1u << 31), "bad dimensions");
    POGS_CHECK(opt->projector == POGS_AMD_PROJ_CGLS_FUSED,
               "a mixed dense handle runs the one-pass CGLS projector: opt->projector must be POGS_AMD_PROJ_CGLS_FUSED "
               "(the direct projector over a float copy: PogsAmdCreateDense with POGS_AMD_STORE_F32)");
    POGS_CHECK(PogsAmdOptStorage(opt) == POGS_AMD_STORE_SAME || PogsAmdOptStorage(opt) == POGS_AMD_STORE_F32,
               "storage: unknown value (a mixed dense handle takes 0 or POGS_AMD_STORE_F32; it keeps the float copy either way)");
    POGS_CHECK(make_mixed_plan(n, 256).ok,
               "the row is too wide for a mixed dense handle (windowed, or past the 10240 columns of the mixed plan's one-pass shapes)");
    PogsAmdOptions o = *opt;
    PogsAmdOptStorage(&o) = POGS_AMD_STORE_F32;
    DeviceGuard guard(o.device);
    new_handle(out, [&] { return make_dense_solver(POGS_AMD_F64, static_cast<int>(ord), m, n, A, mem, &o, nullptr); });
    return 0;
  });
}

int PogsAmdSolve(PogsAmdSolver *s, const void *f_a, const void *f_b, const void *f_c, const void *f_d,
                 const void *f_e, const int *f_h, const void *g_a, const void *g_b, const void *g_c,
                 const void *g_d, const void *g_e, const int *g_h, double rho, double abs_tol, double rel_tol,
                 unsigned int max_iter, unsigned int verbose, int adaptive_rho, int gap_stop, void *x, void *y,
                 void *l, void *mu, double *optval, unsigned int *final_iter) {
  return guarded([&]() {
    POGS_CHECK(s && s->impl, "null solver");
    DeviceGuard guard(s->impl->device());
    const FnHost f = fn_arrays(f_a, f_b, f_c, f_d, f_e, f_h, "f");
    const FnHost g = fn_arrays(g_a, g_b, g_c, g_d, g_e, g_h, "g");
    return s->impl->solve(f, g, make_params(rho, abs_tol, rel_tol, max_iter, verbose, adaptive_rho, gap_stop), x,
                          y, l, mu, optval, final_iter);
  }, s);
}

namespace {
FnHost fn_host(const PogsAmdFn *p) {
  POGS_CHECK(p != nullptr, "null function description");
  FnHost f{p->a, p->b, p->c, p->d, p->e, p->h};
  f.s0[0] = p->a0; f.s0[1] = p->b0; f.s0[2] = p->c0; f.s0[3] = p->d0; f.s0[4] = p->e0;
  f.h0 = p->h0;
  POGS_CHECK(p->h || (p->h0 >= 0 && p->h0 <= 15), "function code out of range");
  return f;
}
// The k function pairs of a multi-problem entry point (first: every f, second: every g), after its null checks;
// `what`: "batched solve" / "many-problem solve", the prefix of its messages.
std::pair<std::vector<FnHost>, std::vector<FnHost>> fn_hosts(const std::string &what, int k, const PogsAmdFn *f,
                                                             const PogsAmdFn *g, const void *x,
                                                             const unsigned *final_iter, const int *status) {
  POGS_CHECK(f && g, (what + ": null function descriptions").c_str());
  POGS_CHECK(x && final_iter && status, (what + ": x, final_iter and status must not be NULL").c_str());
  std::pair<std::vector<FnHost>, std::vector<FnHost>> fg;
  for (int j = 0; j < k; ++j) {
    fg.first.push_back(fn_host(&f[j]));
    fg.second.push_back(fn_host(&g[j]));
  }
  return fg;
}
}  // namespace

int PogsAmdSolveFn(PogsAmdSolver *s, const PogsAmdFn *f, const PogsAmdFn *g, double rho, double abs_tol, double rel_tol,
                   unsigned int max_iter, unsigned int verbose, int adaptive_rho, int gap_stop, void *x, void *y, void *l,
                   void *mu, double *optval, unsigned int *final_iter) {
  return guarded([&]() {
    POGS_CHECK(s && s->impl, "null solver");
    DeviceGuard guard(s->impl->device());
    const FnHost fh = fn_host(f), gh = fn_host(g);
    return s->impl->solve(fh, gh, make_params(rho, abs_tol, rel_tol, max_iter, verbose, adaptive_rho, gap_stop), x, y, l, mu,
                          optval, final_iter);
  }, s);
}

int PogsAmdSolveBatchFn(PogsAmdSolver *s, int k, const PogsAmdFn *f, const PogsAmdFn *g, const double *rho,
                        double abs_tol, double rel_tol, unsigned int max_iter, unsigned int verbose, int adaptive_rho,
                        int gap_stop, void *x, void *y, void *l, void *mu, double *optval, unsigned int *final_iter,
                        int *status) {
  return guarded([&]() {
    POGS_CHECK(s && s->impl, "null solver");
    POGS_CHECK(k >= 1 && k <= POGS_AMD_BATCH_MAX, "batched solve: k must be in [1, POGS_AMD_BATCH_MAX]");
    const auto fg = fn_hosts("batched solve", k, f, g, x, final_iter, status);
    DeviceGuard guard(s->impl->device());
    s->impl->solve_batch(k, fg.first.data(), fg.second.data(), rho,
                         make_params(1.0, abs_tol, rel_tol, max_iter, verbose, adaptive_rho, gap_stop),
                         BatchOut{x, y, l, mu, optval, final_iter, status}, BatchWarm{});
    return 0;
  }, s);
}

int PogsAmdSolveBatchSparseFn(PogsAmdSolver *s, int k, const PogsAmdFn *f, const PogsAmdFn *g, const double *rho,
                              double abs_tol, double rel_tol, unsigned int max_iter, unsigned int verbose,
                              int adaptive_rho, int gap_stop, void *x, void *y, void *l, void *mu, double *optval,
                              unsigned int *final_iter, int *status) {
  return guarded([&]() {
    POGS_CHECK(s && s->impl, "null solver");
    POGS_CHECK(k >= 1 && k <= POGS_AMD_BATCH_MAX, "batched solve: k must be in [1, POGS_AMD_BATCH_MAX]");
    const auto fg = fn_hosts("batched solve", k, f, g, x, final_iter, status);
    DeviceGuard guard(s->impl->device());
    s->impl->solve_batch_sparse(k, fg.first.data(), fg.second.data(), rho,
                                make_params(1.0, abs_tol, rel_tol, max_iter, verbose, adaptive_rho, gap_stop),
                                BatchOut{x, y, l, mu, optval, final_iter, status}, BatchWarm{});
    return 0;
  }, s);
}

int PogsAmdSolveBatchWarmFn(PogsAmdSolver *s, int k, const PogsAmdFn *f, const PogsAmdFn *g, const double *rho,
                            const void *x0, const void *l0, const int *warm, double abs_tol, double rel_tol,
                            unsigned int max_iter, unsigned int verbose, int adaptive_rho, int gap_stop, void *x, void *y,
                            void *l, void *mu, double *optval, unsigned int *final_iter, int *status, double *rho_final) {
  return guarded([&]() {
    POGS_CHECK(s && s->impl, "null solver");
    POGS_CHECK(k >= 1 && k <= POGS_AMD_BATCH_MAX, "batched solve: k must be in [1, POGS_AMD_BATCH_MAX]");
    POGS_CHECK((x0 != nullptr) == (l0 != nullptr), "batched solve: a warm start needs both x0 and l0 (pogs.cpp:159-179)");
    POGS_CHECK(x0 || !warm, "batched solve: warm flags without x0 and l0");
    const auto fg = fn_hosts("batched solve", k, f, g, x, final_iter, status);
    DeviceGuard guard(s->impl->device());
    BatchWarm w;
    w.x0 = x0; w.l0 = l0; w.warm = warm; w.rho_final = rho_final;
    s->impl->solve_batch_any(k, fg.first.data(), fg.second.data(), rho,
                             make_params(1.0, abs_tol, rel_tol, max_iter, verbose, adaptive_rho, gap_stop),
                             BatchOut{x, y, l, mu, optval, final_iter, status}, w);
    return 0;
  }, s);
}

int PogsAmdSolveManyFn(int dtype, enum ORD ord, int k, size_t m, size_t n, const void *A, int mem,
                       const PogsAmdOptions *opt, const PogsAmdFn *f, const PogsAmdFn *g, const double *rho,
                       double abs_tol, double rel_tol, unsigned int max_iter, unsigned int verbose, int adaptive_rho,
                       int gap_stop, void *x, void *y, void *l, void *mu, double *optval, unsigned int *final_iter,
                       int *status) {
  return guarded([&]() {
    check_many_call("many-problem solve", k, opt);
    const int device = opt ? opt->device : -1;
    const auto fg = fn_hosts("many-problem solve", k, f, g, x, final_iter, status);
    DeviceGuard guard(device);
    solve_many(dtype, static_cast<int>(ord), k, m, n, A, mem, device, fg.first.data(), fg.second.data(), rho,
               make_params(1.0, abs_tol, rel_tol, max_iter, verbose, adaptive_rho, gap_stop),
               BatchOut{x, y, l, mu, optval, final_iter, status});
    return 0;
  });
}

int PogsAmdManyCreate(PogsAmdMany **out, int dtype, enum ORD ord, int k, size_t m, size_t n, const void *A, int mem,
                      const PogsAmdOptions *opt) {
  return guarded([&]() {
    POGS_CHECK(out != nullptr, "many-problem handle: null out");
    *out = nullptr;
    check_many_call("many-problem solve", k, opt);
    const int device = opt ? opt->device : -1;
    new_handle(out, [&] { return many_create(dtype, static_cast<int>(ord), k, m, n, A, mem, device); });
    return 0;
  });
}

int PogsAmdSolveManyRaggedFn(int dtype, enum ORD ord, int k, const size_t *m, const size_t *n, const void *A, int mem,
                             const PogsAmdOptions *opt, const PogsAmdFn *f, const PogsAmdFn *g, const double *rho,
                             double abs_tol, double rel_tol, unsigned int max_iter, unsigned int verbose,
                             int adaptive_rho, int gap_stop, void *x, void *y, void *l, void *mu, double *optval,
                             unsigned int *final_iter, int *status) {
  return guarded([&]() {
    check_many_call("ragged many-problem solve", k, opt);
    const int device = opt ? opt->device : -1;
    many_check_ragged(dtype, static_cast<int>(ord), k, m, n, A, mem);
    const auto fg = fn_hosts("ragged many-problem solve", k, f, g, x, final_iter, status);
    DeviceGuard guard(device);
    solve_many_ragged(dtype, static_cast<int>(ord), k, m, n, A, mem, device, fg.first.data(), fg.second.data(), rho,
                      make_params(1.0, abs_tol, rel_tol, max_iter, verbose, adaptive_rho, gap_stop),
                      BatchOut{x, y, l, mu, optval, final_iter, status});
    return 0;
  });
}

int PogsAmdManyCreateRagged(PogsAmdMany **out, int dtype, enum ORD ord, int k, const size_t *m, const size_t *n,
                            const void *A, int mem, const PogsAmdOptions *opt) {
  return guarded([&]() {
    POGS_CHECK(out != nullptr, "many-problem handle: null out");
    *out = nullptr;
    check_many_call("ragged many-problem solve", k, opt);
    const int device = opt ? opt->device : -1;
    new_handle(out, [&] { return many_create_ragged(dtype, static_cast<int>(ord), k, m, n, A, mem, device); });
    return 0;
  });
}

int PogsAmdManyGetShapes(const PogsAmdMany *h, size_t *m, size_t *n) {
  return guarded([&]() {
    POGS_CHECK(h && h->impl && m && n, "null argument");
    h->impl->shapes(m, n);
    return 0;
  });
}

int PogsAmdManySolveFn(PogsAmdMany *h, const PogsAmdFn *f, const PogsAmdFn *g, const double *rho, int start,
                       const void *x0, const void *l0, double abs_tol, double rel_tol, unsigned int max_iter,
                       unsigned int verbose, int adaptive_rho, int gap_stop, void *x, void *y, void *l, void *mu,
                       double *optval, unsigned int *final_iter, int *status, double *rho_final) {
  return guarded([&]() {
    POGS_CHECK(h && h->impl, "many-problem handle: null handle");
    const auto fg = fn_hosts("many-problem handle", h->impl->count(), f, g, x, final_iter, status);
    DeviceGuard guard(h->impl->device());
    h->impl->solve(fg.first.data(), fg.second.data(), ManyStart{start, x0, l0, rho, rho_final},
                   make_params(1.0, abs_tol, rel_tol, max_iter, verbose, adaptive_rho, gap_stop),
                   BatchOut{x, y, l, mu, optval, final_iter, status});
    return 0;
  });
}

int PogsAmdManyGetInfo(const PogsAmdMany *h, PogsAmdManyInfo *out) {
  return guarded([&]() {
    POGS_CHECK(h && h->impl && out, "null argument");
    *out = h->impl->info();
    return 0;
  });
}

void PogsAmdManyDestroy(PogsAmdMany *h) {
  try {
    if (!h) return;
    DeviceGuard guard(h->impl ? h->impl->device() : -1);   // buffers are freed on the handle's device
    delete h;
  } catch (...) {}
}

int PogsAmdBeginRunFn(PogsAmdSolver *s, const PogsAmdFn *f, const PogsAmdFn *g, double rho, double abs_tol, double rel_tol,
                      unsigned int max_iter, int adaptive_rho, int gap_stop) {
  return guarded([&]() {
    POGS_CHECK(s && s->impl, "null solver");
    DeviceGuard guard(s->impl->device());
    const FnHost fh = fn_host(f), gh = fn_host(g);
    s->impl->begin_run(fh, gh, make_params(rho, abs_tol, rel_tol, max_iter, 0, adaptive_rho, gap_stop));
    return 0;
  }, s);
}

int PogsAmdBeginRun(PogsAmdSolver *s, const void *f_a, const void *f_b, const void *f_c, const void *f_d,
                    const void *f_e, const int *f_h, const void *g_a, const void *g_b, const void *g_c,
                    const void *g_d, const void *g_e, const int *g_h, double rho, double abs_tol, double rel_tol,
                    unsigned int max_iter, int adaptive_rho, int gap_stop) {
  return guarded([&]() {
    POGS_CHECK(s && s->impl, "null solver");
    DeviceGuard guard(s->impl->device());
    const FnHost f = fn_arrays(f_a, f_b, f_c, f_d, f_e, f_h, "f");
    const FnHost g = fn_arrays(g_a, g_b, g_c, g_d, g_e, g_h, "g");
    s->impl->begin_run(f, g, make_params(rho, abs_tol, rel_tol, max_iter, 0, adaptive_rho, gap_stop));
    return 0;
  }, s);
}

int PogsAmdIterate(PogsAmdSolver *s, unsigned int iters, double *seconds, unsigned int *solves_completed) {
  return guarded([&]() {
    POGS_CHECK(s && s->impl, "null solver");
    DeviceGuard guard(s->impl->device());
    s->impl->iterate(iters, seconds, solves_completed);
    return 0;
  }, s);
}

int PogsAmdSetWarmStart(PogsAmdSolver *s, const void *x0, const void *l0) {
  return guarded([&]() {
    POGS_CHECK(s && s->impl && x0 && l0, "warm start needs both x0 and l0 (pogs.cpp:159-179)");
    DeviceGuard guard(s->impl->device());
    s->impl->set_warm_start(x0, l0);
    return 0;
  });
}

int PogsAmdGetStats(const PogsAmdSolver *s, PogsAmdStats *out) {
  return guarded([&]() {
    POGS_CHECK(s && s->impl && out, "null argument");
    *out = const_cast<PogsAmdSolver *>(s)->impl->stats();
    return 0;
  });
}

int PogsAmdResetStats(PogsAmdSolver *s) {
  return guarded([&]() {
    POGS_CHECK(s && s->impl, "null solver");
    DeviceGuard guard(s->impl->device());
    PogsAmdStats &st = s->impl->stats();
    st.t_loop_s = 0; st.iterations = 0; st.exact_iters = 0; st.rho_updates = 0;
    st.cg_iters = 0; st.matvecs = 0;
    st.stream_ms = 0; st.stream_launches = 0; st.stream_bytes = 0;
    st.reserved[0] = 0; st.reserved[1] = 0;
    return 0;
  });
}

void PogsAmdDestroy(PogsAmdSolver *s) {
  try {
    if (!s) return;
    DeviceGuard guard(s->impl ? s->impl->device() : -1);   // buffers are freed on the handle's device
    delete s;
  } catch (...) {}
}

const char *PogsAmdLastError(void) { return g_last_error.c_str(); }

int PogsAmdPoolStats(int device, PogsAmdPoolInfo *out) {
  return guarded([&]() {
    POGS_CHECK(out, "null argument");
    int dev = device;
    if (dev < 0) POGS_HIP_CHECK(hipGetDevice(&dev));
    const PoolCounters c = DevicePool::get().counters(dev);
    out->mallocs = c.mallocs; out->reuses = c.reuses; out->frees = c.frees;
    out->malloc_ms = c.malloc_ms; out->free_ms = c.free_ms;
    out->cached_bytes = c.cached_bytes; out->live_bytes = c.live_bytes;
    out->peak_cached_bytes = c.peak_cached_bytes;
    return 0;
  });
}

int PogsAmdPoolTrim(int device, size_t *freed_bytes) {
  return guarded([&]() {
    const size_t b = DevicePool::get().trim(device);
    if (freed_bytes) *freed_bytes = b;
    return 0;
  });
}

int PogsAmdProxEval(int dtype, size_t n, const int *h, const void *a, const void *b, const void *c, const void *d,
                    const void *e, double rho, const void *in, void *out) {
  return guarded([&]() {
    if (dtype == POGS_AMD_F32) prox_eval_host<float>(n, h, a, b, c, d, e, rho, in, out, nullptr);
    else prox_eval_host<double>(n, h, a, b, c, d, e, rho, in, out, nullptr);
    return 0;
  });
}

int PogsAmdFuncEval(int dtype, size_t n, const int *h, const void *a, const void *b, const void *c, const void *d,
                    const void *e, const void *in, double *out) {
  return guarded([&]() {
    if (dtype == POGS_AMD_F32) prox_eval_host<float>(n, h, a, b, c, d, e, 1.0, in, nullptr, out);
    else prox_eval_host<double>(n, h, a, b, c, d, e, 1.0, in, nullptr, out);
    return 0;
  });
}

int PogsAmdProjSubgradEval(int dtype, size_t n, const int *h, const void *a, const void *b, const void *c,
                           const void *d, const void *e, const void *x_in, const void *v_in, void *v_out) {
  return guarded([&]() {
    POGS_CHECK(x_in && v_in && v_out, "null argument");
    if (dtype == POGS_AMD_F32) prox_eval_host<float>(n, h, a, b, c, d, e, 1.0, v_in, v_out, nullptr, x_in);
    else prox_eval_host<double>(n, h, a, b, c, d, e, 1.0, v_in, v_out, nullptr, x_in);
    return 0;
  });
}

int PogsAmdGetEquil(const PogsAmdSolver *s, void *A_eq, void *d, void *e, double *nrmA) {
  return guarded([&]() {
    POGS_CHECK(s && s->impl, "null solver");
    DeviceGuard guard(s->impl->device());
    const_cast<PogsAmdSolver *>(s)->impl->get_equil(A_eq, d, e, nrmA);
    return 0;
  });
}

int PogsAmdProject(PogsAmdSolver *s, const void *x0, const void *y0, double tol, void *x, void *y) {
  return guarded([&]() {
    POGS_CHECK(s && s->impl, "null solver");
    DeviceGuard guard(s->impl->device());
    s->impl->project(x0, y0, tol, x, y);
    return 0;
  });
}

int PogsAmdMul(PogsAmdSolver *s, char trans, double alpha, const void *x, double beta, void *y) {
  return guarded([&]() {
    POGS_CHECK(s && s->impl, "null solver");
    DeviceGuard guard(s->impl->device());
    s->impl->mul(trans, alpha, x, beta, y);
    return 0;
  });
}

int PogsAmdReadBandwidth(int device, size_t bytes, int reps, double *gb_per_s, int *pattern) {
  return guarded([&]() {
    POGS_CHECK(gb_per_s && bytes >= (1u << 20), "null argument / fewer than 1 MiB");
    DeviceGuard guard(device);
    int pat = 0;
    *gb_per_s = measure_read_bandwidth_gbs(bytes, reps, &pat);
    if (pattern) *pattern = pat;
    return 0;
  });
}

int PogsAmdWaveSumCheck(int dtype, size_t n, const void *in_host, void *alu_host, void *lds_host) {
  return guarded([&]() {
    POGS_CHECK(in_host && alu_host && lds_host, "null argument");
    if (dtype == POGS_AMD_F32) wave_sum_check(static_cast<const float *>(in_host), n, static_cast<float *>(alu_host), static_cast<float *>(lds_host));
    else wave_sum_check(static_cast<const double *>(in_host), n, static_cast<double *>(alu_host), static_cast<double *>(lds_host));
    return 0;
  });
}

int PogsAmdBlockIdCheck(int grid, int *ids_host, int *group) {
  return guarded([&]() {
    POGS_CHECK(grid > 0 && ids_host && group, "null argument / empty grid");
    DevBuf<int> ids(static_cast<size_t>(grid));
    hipLaunchKernelGGL(block_id_check_kernel, dim3(grid), dim3(64), 0, nullptr, ids.p);
    POGS_HIP_CHECK(hipGetLastError());
    POGS_HIP_CHECK(hipMemcpy(ids_host, ids.p, static_cast<size_t>(grid) * sizeof(int), hipMemcpyDeviceToHost));
    *group = POGS_XCD_IDS ? kXcdHint : 0;
    return 0;
  });
}

int PogsAmdBatchRowsCheck(int dtype, int tri, int rows, int cols, const void *M, size_t ldm, int k, const int *act,
                          int nact, const void *X, size_t ldx, void *Y, size_t ldy) {
  return guarded([&]() {
    POGS_CHECK(dtype == POGS_AMD_F32 || dtype == POGS_AMD_F64, "unknown dtype");
    if (dtype == POGS_AMD_F32)
      batch_rows_check<float>(tri, rows, cols, static_cast<const float *>(M), ldm, k, act, nact,
                              static_cast<const float *>(X), ldx, static_cast<float *>(Y), ldy);
    else
      batch_rows_check<double>(tri, rows, cols, static_cast<const double *>(M), ldm, k, act, nact,
                               static_cast<const double *>(X), ldx, static_cast<double *>(Y), ldy);
    return 0;
  });
}

int PogsAmdBatchColsCheck(int dtype, int rows, int cols, const void *M, size_t ldm, int k, const int *act, int nact,
                          const void *U, size_t ldu, const void *add, void *Z, size_t ldz, int *nrb_used, int *rpb) {
  return guarded([&]() {
    POGS_CHECK(dtype == POGS_AMD_F32 || dtype == POGS_AMD_F64, "unknown dtype");
    if (dtype == POGS_AMD_F32)
      batch_cols_check<float>(rows, cols, static_cast<const float *>(M), ldm, k, act, nact,
                              static_cast<const float *>(U), ldu, static_cast<const float *>(add),
                              static_cast<float *>(Z), ldz, nrb_used, rpb);
    else
      batch_cols_check<double>(rows, cols, static_cast<const double *>(M), ldm, k, act, nact,
                               static_cast<const double *>(U), ldu, static_cast<const double *>(add),
                               static_cast<double *>(Z), ldz, nrb_used, rpb);
    return 0;
  });
}

int PogsAmdBatchRowsMixedCheck(int rows, int cols, const float *M, size_t ldm, int k, const int *act, int nact,
                               const double *X, size_t ldx, double *Y, size_t ldy) {
  return guarded([&]() {
    batch_rows_mixed_check(rows, cols, M, ldm, k, act, nact, X, ldx, Y, ldy);
    return 0;
  });
}

int PogsAmdBatchColsMixedCheck(int rows, int cols, const float *M, size_t ldm, int k, const int *act, int nact,
                               const double *U, size_t ldu, const double *add, double *Z, size_t ldz, int *nrb_used,
                               int *rpb) {
  return guarded([&]() {
    batch_cols_mixed_check(rows, cols, M, ldm, k, act, nact, U, ldu, add, Z, ldz, nrb_used, rpb);
    return 0;
  });
}

int PogsAmdSpBatchSpmvCheck(int dtype, int nrows, int ncols, const int *ptr, const int *ind, const void *val, int k,
                            const int *act, int nact, const void *X, size_t ldx, double beta, const void *yin,
                            size_t ldin, void *Y, size_t ldy, double *part, int num_cu, int *geom) {
  return guarded([&]() {
    POGS_CHECK(dtype == POGS_AMD_F32 || dtype == POGS_AMD_F64, "unknown dtype");
    if (dtype == POGS_AMD_F32)
      sp_batch_spmv_check<float>(nrows, ncols, ptr, ind, static_cast<const float *>(val), k, act, nact,
                                 static_cast<const float *>(X), ldx, static_cast<float>(beta),
                                 static_cast<const float *>(yin), ldin, static_cast<float *>(Y), ldy, part, num_cu,
                                 geom);
    else
      sp_batch_spmv_check<double>(nrows, ncols, ptr, ind, static_cast<const double *>(val), k, act, nact,
                                  static_cast<const double *>(X), ldx, beta, static_cast<const double *>(yin), ldin,
                                  static_cast<double *>(Y), ldy, part, num_cu, geom);
    return 0;
  });
}

int PogsAmdManySetupCheck(int dtype, enum ORD ord, int k, size_t m, size_t n, const void *A, int mem, void *A_eq,
                          void *d, void *e, double *nrmA, void *W) {
  return guarded([&]() {
    many_setup_check(dtype, static_cast<int>(ord), k, m, n, A, mem, A_eq, d, e, nrmA, W);
    return 0;
  });
}

int PogsAmdGramCheck(int dtype, int kdim, int k, const void *P, size_t lda, int num_cu, int force, void *G, size_t ldg,
                     int *info) {
  return guarded([&]() {
    POGS_CHECK(dtype == POGS_AMD_F32 || dtype == POGS_AMD_F64, "unknown dtype");
    if (dtype == POGS_AMD_F32)
      gram_check<float>(kdim, k, static_cast<const float *>(P), lda, num_cu, force, static_cast<float *>(G), ldg, info);
    else
      gram_check<double>(kdim, k, static_cast<const double *>(P), lda, num_cu, force, static_cast<double *>(G), ldg, info);
    return 0;
  });
}

int PogsAmdDensePassCheck(const PogsAmdDensePassArgs *args) {
  return guarded([&]() {
    dense_pass_check(args);
    return 0;
  });
}

int PogsAmdDensePassMixedCheck(const PogsAmdDensePassArgs *args) {
  return guarded([&]() {
    dense_pass_mixed_check(args);
    return 0;
  });
}

int PogsAmdVecCheck(const PogsAmdVecArgs *args) {
  return guarded([&]() {
    vec_check(args);
    return 0;
  });
}

int PogsAmdCholCheck(int dtype, int n, const void *H, size_t ldh, void *L, void *W, void *U, size_t ldo) {
  return guarded([&]() {
    POGS_CHECK(dtype == POGS_AMD_F32 || dtype == POGS_AMD_F64, "unknown dtype");
    if (dtype == POGS_AMD_F32)
      chol_check<float>(n, static_cast<const float *>(H), ldh, static_cast<float *>(L), static_cast<float *>(W),
                        static_cast<float *>(U), ldo);
    else
      chol_check<double>(n, static_cast<const double *>(H), ldh, static_cast<double *>(L), static_cast<double *>(W),
                         static_cast<double *>(U), ldo);
    return 0;
  });
}

int PogsAmdSpmvCheck(int dtype, enum ORD ord, int nrows, int ncols, const int *ptr, const int *ind, const void *val,
                     int num_cu, int format, int force_rr_rows, int force_ncg, double scale, char trans, int sq,
                     double x_nrm2, double alpha, double beta, const void *x, size_t xlen, void *y, size_t ylen,
                     double *sumsq, int *info, int *t_ptr, int *t_ind, void *t_val) {
  return guarded([&]() {
    const SpmvCheckArgs a{dtype, static_cast<int>(ord), nrows, ncols, ptr, ind, val, num_cu, format, force_rr_rows,
                          force_ncg, scale, trans, sq, x_nrm2, alpha, beta, x, xlen, y, ylen, sumsq, info, t_ptr, t_ind,
                          t_val, 0};
    spmv_check(a);
    return 0;
  });
}

int PogsAmdSpmvMixedCheck(enum ORD ord, int nrows, int ncols, const int *ptr, const int *ind, const double *val, int num_cu,
                          int format, int force_rr_rows, int force_ncg, double scale, char trans, double x_nrm2,
                          double alpha, double beta, const double *x, size_t xlen, double *y, size_t ylen, double *sumsq,
                          int *info) {
  return guarded([&]() {
    const SpmvCheckArgs a{POGS_AMD_F64, static_cast<int>(ord), nrows, ncols, ptr, ind, val, num_cu, format, force_rr_rows,
                          force_ncg, scale, trans, 0, x_nrm2, alpha, beta, x, xlen, y, ylen, sumsq, info, nullptr, nullptr,
                          nullptr, 1};
    spmv_check(a);
    return 0;
  });
}

int PogsAmdSparseCgCheck(PogsAmdSolver *s, const void *x0, const void *y0, const void *x_warm, const void *y_warm,
                         const void *x_prev, const void *x12, const void *y12, double tol, int max_steps, int ahead,
                         int ysync, int loop, void *x, void *y_new, void *xtemp, void *ytemp, void *r, void *p, void *sv,
                         double *slots, double *rec_x, int *info, int *enqueued) {
  return guarded([&]() {
    // every refusal comes before the first HIP call (the handle's own: a dense one, row shards, copies not tiled)
    POGS_CHECK(x0 && y0 && x_warm && y_warm && x_prev && x12 && y12 && x && y_new && xtemp && ytemp && r && p && sv &&
                   slots && rec_x && info && enqueued,
               "null argument");
    POGS_CHECK(loop >= 0 && loop <= 2, "loop must be 0 (device-resident), 1 (host-polled, warm) or 2 (host-polled, cold)");
    POGS_CHECK(ysync == 0 || ysync == 1, "ysync must be 0 or 1");
    POGS_CHECK(ahead >= 1, "ahead must be >= 1");
    POGS_CHECK(max_steps >= 1, "max_steps must be >= 1");
    POGS_CHECK(s && s->impl, "null solver");
    DeviceGuard guard(s->impl->device());
    s->impl->sparse_cg_check(SparseCgCheckArgs{x0, y0, x_warm, y_warm, x_prev, x12, y12, tol, max_steps, ahead, ysync, loop,
                                               x, y_new, xtemp, ytemp, r, p, sv, slots, rec_x, info, enqueued});
    return 0;
  });
}

int PogsAmdStreamMixedCheck(int form, int rows, int n, const float *M, size_t ldm, int num_cu, int force_tpb, int force_nv,
                            const double *x, const double *u, double done, double *q, double *tot, double *scalars,
                            double *partials, size_t partials_len, int *info) {
  return guarded([&]() {
    stream_mixed_check(StreamMixedCheckArgs{form, rows, n, M, ldm, num_cu, force_tpb, force_nv, x, u, done, q, tot, scalars,
                                            partials, partials_len, info});
    return 0;
  });
}

int PogsAmdDenseCgCheck(PogsAmdSolver *s, const void *x0, const void *y0, const void *x_warm, const void *y_warm,
                        double tol, int max_steps, int ahead, int ysync, void *x, void *y_new, void *r, void *p, void *sv,
                        double *slots, int *enqueued, int *steps, unsigned long long *matvecs) {
  return guarded([&]() {
    // every refusal comes before the first HIP call (the handle's own: any handle but a dense fused one)
    POGS_CHECK(x0 && y0 && x_warm && y_warm && x && y_new && r && p && sv && slots && enqueued && steps && matvecs,
               "null argument");
    POGS_CHECK(ysync == 0 || ysync == 1, "ysync must be 0 or 1");
    POGS_CHECK(ahead >= 1, "ahead must be >= 1");
    POGS_CHECK(max_steps >= 1, "max_steps must be >= 1");
    POGS_CHECK(s && s->impl, "null solver");
    if (!s->impl->has_dense_cg_fused()) throw Error("PogsAmdDenseCgCheck needs a dense handle created with POGS_AMD_PROJ_CGLS_FUSED");
    DeviceGuard guard(s->impl->device());
    s->impl->dense_cg_check(DenseCgCheckArgs{x0, y0, x_warm, y_warm, tol, max_steps, ahead, ysync, x, y_new, r, p, sv, slots,
                                             enqueued, steps, matvecs});
    return 0;
  });
}

int PogsAmdSparseGramCheck(int dtype, enum ORD ord, int nrows, int ncols, const int *ptr, const int *ind,
                           const void *val, int num_cu, int window, void *G, size_t ldg, int *info) {
  return guarded([&]() {
    sparse_gram_check(SparseGramCheckArgs{dtype, static_cast<int>(ord), nrows, ncols, ptr, ind, val, num_cu, window, G,
                                          ldg, info});
    return 0;
  });
}

int PogsAmdTriMatvecCheck(int dtype, int tri, int n, const void *M, size_t ldm, const void *x, void *y) {
  return guarded([&]() {
    tri_matvec_check(dtype, tri, n, M, ldm, x, y);
    return 0;
  });
}

int PogsAmdGetFactor(const PogsAmdSolver *s, void *W, void *U) {
  return guarded([&]() {
    POGS_CHECK(s && s->impl, "null solver");
    DeviceGuard guard(s->impl->device());
    const_cast<PogsAmdSolver *>(s)->impl->get_factor(W, U);
    return 0;
  });
}

int PogsAmdRandUniform(int dtype, size_t n, void *out_host) {
  return guarded([&]() {
    if (dtype == POGS_AMD_F32) rand_uniform_host(static_cast<float *>(out_host), n);
    else rand_uniform_host(static_cast<double *>(out_host), n);
    return 0;
  });
}

}  // extern "C"

// Many small dense problems, each with its own matrix (PogsAmdSolveManyFn, include/pogs_amd.h).
//
// One workgroup owns one problem from setup to epilogue: it copies and equilibrates its A_j, estimates its norm,
// factors I + A^T A (m > n) or I + A A^T (m <= n), inverts the Cholesky factor (W = L^-1), and runs the two-pass
// ADMM iteration of pogs.cpp with the stopping rule and adaptive rho of AdmmControl (engine.h) on the device.  Only
// the Gram matrix is formed by several workgroups per problem (one 64 x 64 tile each).  Problems never talk to each
// other, so there is no host poll per iteration: a loop launch advances every live problem by at most a fixed number
// of iterations, keeps its state in device memory, and the host reads back one done-count per launch.
//
// Every sum inside a problem runs in a fixed order that depends on (m, n) alone (fixed thread -> element maps,
// fixed butterflies, partials combined in index order), and a problem's arithmetic never looks at its index, the
// chunk or the other problems: its bytes are its own.
//
// The ragged entries (PogsAmdSolveManyRaggedFn / PogsAmdManyCreateRagged) give every problem its own shape: a table
// with one row per problem (ManyProb) tells each workgroup its (m, n) and where its data lives, and many_problem(),
// called once at the top of every kernel, turns the kernel's arguments into that problem's; the code below it is the
// same for both layouts.
//
// The persistent handle (PogsAmdManyCreate / PogsAmdManySolveFn) runs the same setup once, keeps all k problems
// resident and opens every solve with many_begin_kernel: cold, or warm from a problem's kept x, l and rho.
//
// The kernels and their argument structs are in many_device.h, the arithmetic on shapes (workspace layout, prefix sums,
// chunks) in many_plan.h; below is the host driver: ManySet, the device buffers of a set of resident problems, the
// staging of A, the two launch sequences, the one-shot solve, the handle and the entries.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "many_device.h"
#include "many_kernels.h"

namespace pogs_amd {

void rand_uniform_host(float *x, size_t n);    // abi.hip: the Norm2Est start vector (gsl_rand.h:8-16)
void rand_uniform_host(double *x, size_t n);

namespace {

size_t workspace_cap_bytes(int device) {
  const char *env = std::getenv("POGS_AMD_MANY_WORKSPACE_MB");
  if (env && env[0]) {
    const double mb = std::atof(env);
    if (mb > 0) return static_cast<size_t>(mb * (1 << 20));
  }
  size_t total = 0;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess) total = prop.totalGlobalMem;
  return total ? total / 8 : (size_t(4) << 30);
}

// The shape fields of ManyArgs: the problem's workspace layout (offsets in elements of T) and the Sinkhorn-Knopp
// regularisers (equil_helper.h:152-153, 159-160).
template <typename T>
void many_layout(ManyArgs<T> &a, int ord, size_t m_, size_t n_) {
  many_offsets(a, static_cast<int>(m_), static_cast<int>(n_));
  a.rowmaj = ord == ROW_MAJ;
  a.ce = static_cast<T>(1e-4) * static_cast<T>(m_ + n_) / static_cast<T>(m_);
  a.cd = static_cast<T>(1e-4) * static_cast<T>(m_ + n_) / static_cast<T>(n_);
}

// The Norm2Est start vector (n values) on the device.
template <typename T>
DevBuf<T> many_start_vector(size_t n, hipStream_t s) {
  std::vector<T> r(n);
  rand_uniform_host(r.data(), n);
  DevBuf<T> rnd(n);
  POGS_HIP_CHECK(hipMemcpyAsync(rnd.p, r.data(), n * sizeof(T), hipMemcpyHostToDevice, s));
  POGS_HIP_CHECK(hipStreamSynchronize(s));
  return rnd;
}

// The setup of the cnt problems of a chunk (a: many_layout's fields, ws, st, src and rnd set): zero workspaces and
// states, then copy, all 50 Sinkhorn-Knopp passes, scale, norm estimate, Gram tiles, factor and W = L^-1.  Returns the
// number of launches.  The solve and PogsAmdManySetupCheck both run this sequence.
// x: the problems' extent (many_extent); the launches are cut by the largest matrix and the Gram grid covers the
// largest order.  ws0: where the cnt workspaces start (a.ws for a uniform chunk).
template <typename T>
unsigned long long many_setup(const ManyArgs<T> &a, int cnt, const ManyExtent &x, T *ws0, hipStream_t s) {
  const size_t mn = x.mn_max;
  const int K = x.K_max;
  const double pass_bytes = 2.0 * static_cast<double>(mn) * sizeof(T);
  const int per_launch = static_cast<int>(std::max(1.0, std::min(50.0, kLaunchBytes / pass_bytes)));
  const int nb = (K + 63) / 64, ntiles = nb * (nb + 1) / 2;
  const int copy_blocks = static_cast<int>(std::min<size_t>(64, (mn + kTPB - 1) / kTPB));
  unsigned long long launches = 0;
  POGS_HIP_CHECK(hipMemsetAsync(a.st, 0, static_cast<size_t>(cnt) * sizeof(ManyState<T>), s));
  // zero work vectors: the cold start (z = zt = 0)
  POGS_HIP_CHECK(hipMemsetAsync(ws0, 0, x.ws_elems * sizeof(T), s));
  hipLaunchKernelGGL(many_copy_kernel<T>, dim3(copy_blocks, cnt), dim3(kTPB), 0, s, a);
  ++launches;
  for (int p0 = 0; p0 < 50; p0 += per_launch) {
    hipLaunchKernelGGL(many_sk_kernel<T>, dim3(cnt), dim3(kTPB), 0, s, a, p0, std::min(per_launch, 50 - p0));
    ++launches;
  }
  hipLaunchKernelGGL(many_scale_kernel<T>, dim3(cnt), dim3(kTPB), 0, s, a);
  ++launches;
  for (int i0 = 0; i0 < 50; i0 += per_launch) {
    hipLaunchKernelGGL(many_normest_kernel<T>, dim3(cnt), dim3(kTPB), 0, s, a, i0, std::min(per_launch, 50 - i0));
    ++launches;
  }
  hipLaunchKernelGGL(many_gram_kernel<T>, dim3(ntiles, cnt), dim3(kTPB), 0, s, a);
  hipLaunchKernelGGL(many_factor_kernel<T>, dim3(cnt), dim3(kTPB), 0, s, a);
  launches += 2;
  POGS_HIP_CHECK(hipGetLastError());
  return launches;
}

// The functions of cnt problems on their way to the device: per-element fields packed into one upload (tpool, hpool),
// broadcast fields as values.  The host copies live here until the next run.
template <typename T>
struct ManyFnUpload {
  std::vector<T> tp;
  std::vector<int> hp;
  std::vector<ManyFn<T>> fh;
  void run(const FnHost *f, const FnHost *g, const ManyShapes<T> &sh, size_t j0, int cnt, T *tpool, int *hpool,
           ManyFn<T> *fnd, hipStream_t s) {
    tp.clear();
    hp.clear();
    fh.resize(2 * static_cast<size_t>(cnt));
    for (int q = 0; q < cnt; ++q) {
      for (int side = 0; side < 2; ++side) {
        const FnHost &fn = side == 0 ? f[j0 + q] : g[j0 + q];
        const size_t len = side == 0 ? sh.m(j0 + q) : sh.n(j0 + q);
        warn_negative_coeffs<T>(fn, len);
        ManyFn<T> &d = fh[2 * q + side];
        const void *ptr[5] = {fn.a, fn.b, fn.c, fn.d, fn.e};
        for (int fld = 0; fld < 5; ++fld) {
          d.v[fld] = static_cast<T>(fn.s0[fld]);
          d.p[fld] = nullptr;
          if (ptr[fld]) {
            d.p[fld] = tpool + tp.size();
            const T *src_f = static_cast<const T *>(ptr[fld]);
            tp.insert(tp.end(), src_f, src_f + len);
          }
        }
        d.h0 = fn.h0;
        d.h = nullptr;
        if (fn.h) {
          d.h = hpool + hp.size();
          hp.insert(hp.end(), fn.h, fn.h + len);
        }
      }
    }
    if (!tp.empty()) POGS_HIP_CHECK(hipMemcpyAsync(tpool, tp.data(), tp.size() * sizeof(T), hipMemcpyHostToDevice, s));
    if (!hp.empty()) POGS_HIP_CHECK(hipMemcpyAsync(hpool, hp.data(), hp.size() * sizeof(int), hipMemcpyHostToDevice, s));
    POGS_HIP_CHECK(hipMemcpyAsync(fnd, fh.data(), 2 * static_cast<size_t>(cnt) * sizeof(ManyFn<T>), hipMemcpyHostToDevice,
                                  s));
  }
};

// A's way to the kernels, chunk by chunk (starts: many_chunks): a device A is read where it is, a host A goes through
// one staging buffer that holds the largest chunk.
template <typename T>
struct ManyStage {
  const ManyShapes<T> &sh;
  const T *A;
  bool host;
  DevBuf<T> buf;
  ManyStage(const ManyShapes<T> &shapes, const void *Ain, int mem, const std::vector<size_t> &starts)
      : sh(shapes), A(static_cast<const T *>(Ain)), host(mem == POGS_AMD_HOST) {
    size_t el = 0;
    for (size_t c = 0; host && c + 1 < starts.size(); ++c)
      el = std::max(el, sh.els(starts[c], starts[c + 1] - starts[c]));
    buf.alloc(el);
  }
  // the matrices of problems [j0, j0 + cnt) on the device (a host A: their upload is on s)
  const T *chunk(size_t j0, size_t cnt, hipStream_t s) const {
    const T *src = A + sh.el0(j0);
    if (!host) return src;
    POGS_HIP_CHECK(hipMemcpyAsync(buf.p, src, sh.els(j0, cnt) * sizeof(T), hipMemcpyHostToDevice, s));
    return buf.p;
  }
};

// The device buffers of up to cnt resident problems, slot q of every per-problem array and the packed rows / columns
// / workspaces in slot order: the one-shot solve keeps one set for its largest chunk, the handle one for all k.
template <typename T>
struct ManySet {
  DevBuf<T> ws, xo, yo, lo, muo, tpool;
  DevBuf<ManyProb<T>> prob;                // ragged: the table
  DevBuf<double> optv;
  DevBuf<unsigned> iters, done;
  DevBuf<int> stat, hpool, warm;           // warm: the handle's warm-start flags
  DevBuf<ManyFn<T>> fn;
  DevBuf<AdmmControl<T>> ctl;
  DevBuf<ManyState<T>> st;
  PinnedBuf<unsigned> hdone;               // the done count as the host reads it after every loop launch
  ManyFnUpload<T> up;
  std::vector<AdmmControl<T>> ch;          // the control blocks' host copy

  // What many_setup touches: workspaces and states (PogsAmdManySetupCheck reserves no more).
  void reserve_setup(size_t cnt, size_t ws_e) {
    ws.alloc(ws_e);
    st.alloc(cnt);
  }
  // Everything, for cnt problems of `rows` rows, `cols` columns and ws_e workspace elements in all.
  void reserve(size_t cnt, size_t rows, size_t cols, size_t ws_e, bool table, bool warm_flags) {
    reserve_setup(cnt, ws_e);
    xo.alloc(cols); yo.alloc(rows); lo.alloc(rows); muo.alloc(cols);
    optv.alloc(cnt); iters.alloc(cnt); stat.alloc(cnt); done.alloc(1);
    if (warm_flags) warm.alloc(cnt);
    fn.alloc(2 * cnt); ctl.alloc(cnt);
    tpool.alloc(5 * (rows + cols) + 1); hpool.alloc(rows + cols + 1);
    if (table) prob.alloc(cnt);
    hdone.alloc(1);
  }
  // The bytes both footprints below count for what reserve() takes (len = rows + cols): workspace, the four outputs,
  // the five coefficient arrays and the codes, and per problem the control block, the state and the table row.
  static size_t bytes(size_t cnt, size_t len, size_t ws_e, bool table) {
    return sizeof(T) * (ws_e + 2 * len + 5 * len) + sizeof(int) * len +
           cnt * (sizeof(AdmmControl<T>) + sizeof(ManyState<T>) + (table ? sizeof(ManyProb<T>) : 0));
  }
  // What the one-shot solve's chunk plan charges one problem: its staged matrix too (a host A), and a flat 64 bytes
  // for the small per-problem arrays.
  static size_t chunk_bytes(size_t len, size_t ws_e, size_t stage_e, bool table) {
    return bytes(1, len, ws_e, table) + sizeof(T) * stage_e + 64;
  }
  // PogsAmdManyInfo::resident_bytes of a handle: the small arrays counted out (status, warm flags, optval, iterations,
  // the two function headers) and one T per problem, which the figure has always included.
  static size_t resident_bytes(size_t cnt, size_t len, size_t ws_e, bool table) {
    return bytes(cnt, len, ws_e, table) +
           cnt * (sizeof(T) + 2 * sizeof(int) + sizeof(double) + sizeof(unsigned) + 2 * sizeof(ManyFn<T>));
  }

  // The set's pointers into a (what was not reserved stays null); the caller sets src, rnd and the layout.
  void wire(ManyArgs<T> &a) const {
    a.ws = ws.p; a.fn = fn.p; a.ctl = ctl.p; a.st = st.p; a.done_count = done.p;
    a.xo = xo.p; a.yo = yo.p; a.lo = lo.p; a.muo = muo.p; a.optval = optv.p; a.iters = iters.p; a.status = stat.p;
    a.prob = prob.p;
  }
  // Opens a run of problems [j0, j0 + cnt) in slots 0 .. cnt - 1: their functions and control blocks (rho: indexed as f
  // and g are; null: 1.0 each) go up and the done counter is zeroed, all on s.
  void open(const FnHost *f, const FnHost *g, const ManyShapes<T> &sh, size_t j0, int cnt, const SolveParams &p,
            const double *rho, hipStream_t s) {
    up.run(f, g, sh, j0, cnt, tpool.p, hpool.p, fn.p, s);
    ch.resize(static_cast<size_t>(cnt));
    for (int q = 0; q < cnt; ++q)
      ch[q] = make_admm_control<T>(p, rho ? rho[j0 + q] : 1.0, sh.m(j0 + q), sh.n(j0 + q));
    POGS_HIP_CHECK(hipMemcpyAsync(ctl.p, ch.data(), static_cast<size_t>(cnt) * sizeof(AdmmControl<T>),
                                  hipMemcpyHostToDevice, s));
    POGS_HIP_CHECK(hipMemsetAsync(done.p, 0, sizeof(unsigned), s));
  }
  // The outputs of slots 0 .. cnt - 1 into out at problems [j0, j0 + cnt), on s (the caller synchronises).
  void fetch(const ManyShapes<T> &sh, size_t j0, size_t cnt, const BatchOut &out, hipStream_t s) const {
    auto d2h = [&](void *dst, const void *srcd, size_t bytes) {
      POGS_HIP_CHECK(hipMemcpyAsync(dst, srcd, bytes, hipMemcpyDeviceToHost, s));
    };
    const size_t xb = sh.cols(j0, cnt) * sizeof(T), yb = sh.rows(j0, cnt) * sizeof(T);
    d2h(static_cast<T *>(out.x) + sh.col0(j0), xo.p, xb);
    if (out.y) d2h(static_cast<T *>(out.y) + sh.row0(j0), yo.p, yb);
    if (out.l) d2h(static_cast<T *>(out.l) + sh.row0(j0), lo.p, yb);
    if (out.mu) d2h(static_cast<T *>(out.mu) + sh.col0(j0), muo.p, xb);
    if (out.optval) d2h(out.optval + j0, optv.p, cnt * sizeof(double));
    d2h(out.final_iter + j0, iters.p, cnt * sizeof(unsigned));
    d2h(out.status + j0, stat.p, cnt * sizeof(int));
  }
};

// PogsAmdManySetupCheck: many_setup on k problems in one chunk, then per problem A_eq, d, e, nrmA and W (K x K).
template <typename T>
void many_setup_check_t(int ord, int kk, size_t m_, size_t n_, const void *Ain, int mem, T *A_eq, T *d, T *e,
                        double *nrmA, T *W) {
  Ctx ctx;
  ctx.init(-1, 0);
  hipStream_t s = ctx.stream;
  const size_t kz = static_cast<size_t>(kk), mn = m_ * n_;
  ManyShapes<T> sh;
  sh.set_uniform(kk, m_, n_);
  ManyArgs<T> a{};
  many_layout(a, ord, m_, n_);
  const size_t K = static_cast<size_t>(a.k);
  ManySet<T> set;
  set.reserve_setup(kz, sh.wss(0, kz));
  set.wire(a);
  const ManyStage<T> stage(sh, Ain, mem, {0, kz});
  const DevBuf<T> rnd = many_start_vector<T>(n_, s);
  a.rnd = rnd.p;
  a.src = stage.chunk(0, kz, s);
  many_setup(a, kk, many_extent(sh, 0, kz), set.ws.p, s);
  std::vector<ManyState<T>> hst(kz);
  POGS_HIP_CHECK(hipMemcpyAsync(hst.data(), set.st.p, kz * sizeof(ManyState<T>), hipMemcpyDeviceToHost, s));
  for (size_t q = 0; q < kz; ++q) {
    const T *w = set.ws.p + sh.ws0(q);
    auto d2h = [&](T *dst, size_t off, size_t len) {
      if (dst) POGS_HIP_CHECK(hipMemcpyAsync(dst + q * len, w + off, len * sizeof(T), hipMemcpyDeviceToHost, s));
    };
    d2h(A_eq, a.oA, mn);
    d2h(d, a.oy[kD], m_);
    d2h(e, a.ox[kE], n_);
    d2h(W, a.oW, K * K);
  }
  POGS_HIP_CHECK(hipStreamSynchronize(s));
  if (nrmA)
    for (size_t q = 0; q < kz; ++q) nrmA[q] = static_cast<double>(hst[q].nrmA);
}

// The loop of cnt problems (a.done_count zeroed on the stream before): every launch advances each live problem by at
// most its own iterations per launch (x.ipl_max is the launch's bound, a ragged problem's table row may lower it;
// x.ipl_min bounds the number of launches), and the host reads one done-count per launch.  Returns the number of
// launches.
template <typename T>
unsigned long long many_run_loop(const ManyArgs<T> &a, int cnt, const ManyExtent &x, unsigned max_iter,
                                 unsigned *hdone, hipStream_t s) {
  const unsigned long long max_launches = (max_iter + x.ipl_min - 1) / x.ipl_min + 1;
  unsigned long long nl = 0;
  for (;;) {
    hipLaunchKernelGGL(many_loop_kernel<T>, dim3(cnt), dim3(kTPB), 0, s, a, x.ipl_max);
    POGS_HIP_CHECK(hipGetLastError());
    ++nl;
    POGS_HIP_CHECK(hipMemcpyAsync(hdone, a.done_count, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    POGS_HIP_CHECK(hipStreamSynchronize(s));
    if (*hdone >= static_cast<unsigned>(cnt)) break;
    POGS_CHECK(nl < max_launches, "many-problem solve: a problem did not stop within max_iter iterations");
  }
  return nl;
}

// The one summary line of a call (verbose > 0).  head: what precedes "; status".
inline void many_print_summary(const char *head, int k, const unsigned *final_iter, const int *status, double t_setup,
                               double t_loop, double t_total, unsigned long long launches) {
  int counts[7] = {0, 0, 0, 0, 0, 0, 0};
  unsigned it_lo = ~0u, it_hi = 0;
  for (int q = 0; q < k; ++q) {
    const int st = status[q];
    ++counts[st >= 0 && st < 7 ? st : 6];
    it_lo = std::min(it_lo, final_iter[q]);
    it_hi = std::max(it_hi, final_iter[q]);
  }
  std::printf("%s; status", head);
  for (int st = 0; st < 7; ++st)
    if (counts[st]) std::printf(" %s: %d,", status_string(st), counts[st]);
  std::printf(" iterations %u..%u; setup %.3e s, loop %.3e s, total %.3e s; %llu launches\n", it_lo, it_hi, t_setup,
              t_loop, t_total, launches);
  std::fflush(stdout);
}

// "of 500 x 300" or, ragged, "of 310..700 x 300..300": the shapes in a summary line.
template <typename T>
void many_shape_text(char *buf, size_t len, const ManyShapes<T> &sh) {
  if (!sh.ragged) {
    std::snprintf(buf, len, "%zu x %zu", sh.m0, sh.n0);
    return;
  }
  std::snprintf(buf, len, "%zu..%zu x %zu..%zu", *std::min_element(sh.mv.begin(), sh.mv.end()), sh.m0,
                *std::min_element(sh.nv.begin(), sh.nv.end()), sh.n0);
}

// The one-shot solve of the sh.k problems, uniform or ragged, in chunks under the workspace cap.
template <typename T>
void solve_many_t(int ord, const ManyShapes<T> &sh, const void *Ain, int mem, int device, const FnHost *f,
                  const FnHost *g, const double *rho0, const SolveParams &p, const BatchOut &out) {
  const double t0 = wall_s();
  Ctx ctx;
  ctx.init(device, 0);
  hipStream_t s = ctx.stream;
  const size_t kz = static_cast<size_t>(sh.k);
  const bool host = mem == POGS_AMD_HOST;
  const std::vector<size_t> starts = many_chunks(kz, workspace_cap_bytes(ctx.device), kz, [&](size_t j) {
    return ManySet<T>::chunk_bytes(sh.m(j) + sh.n(j), sh.wss(j, 1), host ? sh.els(j, 1) : 0, sh.ragged);
  });
  // every buffer holds the largest chunk
  size_t chunk = 0, ws_e = 0, rows = 0, cols = 0;
  for (size_t c = 0; c + 1 < starts.size(); ++c) {
    const size_t j0 = starts[c], cnt = starts[c + 1] - j0;
    chunk = std::max(chunk, cnt);
    ws_e = std::max(ws_e, sh.wss(j0, cnt));
    rows = std::max(rows, sh.rows(j0, cnt));
    cols = std::max(cols, sh.cols(j0, cnt));
  }
  ManySet<T> set;
  set.reserve(chunk, rows, cols, ws_e, sh.ragged, false);
  const ManyStage<T> stage(sh, Ain, mem, starts);
  // the start vector of the widest problem: a narrower one reads its first n values, which are what it gets alone
  const DevBuf<T> rnd = many_start_vector<T>(sh.n0, s);
  ManyArgs<T> a{};
  many_layout(a, ord, sh.m0, sh.n0);   // ragged: every kernel replaces the shape fields by the problem's own
  set.wire(a);
  a.rnd = rnd.p;

  std::vector<ManyProb<T>> tab;
  unsigned long long launches = 0;
  double t_setup = 0, t_loop = 0;
  for (size_t c = 0; c + 1 < starts.size(); ++c) {
    const size_t j0 = starts[c];
    const int cnt = static_cast<int>(starts[c + 1] - j0);
    const ManyExtent ext = many_extent(sh, j0, cnt);
    const double tc0 = wall_s();
    a.src = stage.chunk(j0, cnt, s);
    if (sh.ragged) {
      // a chunk's table counts every offset from the chunk's first problem: the set holds the chunk alone
      sh.table(tab, j0, cnt, j0);
      POGS_HIP_CHECK(hipMemcpyAsync(set.prob.p, tab.data(), tab.size() * sizeof(ManyProb<T>), hipMemcpyHostToDevice, s));
    }
    set.open(f, g, sh, j0, cnt, p, rho0, s);
    launches += many_setup(a, cnt, ext, set.ws.p, s);
    ctx.sync();
    const double tc1 = wall_s();
    t_setup += tc1 - tc0;
    // the loop: every launch advances each live problem by at most its iterations per launch
    launches += many_run_loop(a, cnt, ext, p.max_iter, set.hdone.p, s);
    t_loop += wall_s() - tc1;
    set.fetch(sh, j0, cnt, out, s);
    POGS_HIP_CHECK(hipStreamSynchronize(s));
  }
  if (p.verbose > 0) {
    char head[200], shape[96];
    many_shape_text(shape, sizeof(shape), sh);
    if (sh.ragged)
      std::snprintf(head, sizeof(head), "POGS-AMD many: %d ragged problems of %s (%s), %zu chunks of at most %zu", sh.k,
                    shape, sizeof(T) == 8 ? "fp64" : "fp32", starts.size() - 1, chunk);
    else
      std::snprintf(head, sizeof(head), "POGS-AMD many: %d problems of %s (%s), %zu per chunk", sh.k, shape,
                    sizeof(T) == 8 ? "fp64" : "fp32", chunk);
    many_print_summary(head, sh.k, out.final_iter, out.status, t_setup, t_loop, wall_s() - t0, launches);
  }
}


// The persistent handle (PogsAmdMany): setup once for all k problems in one resident workspace, then any number of
// solves, each opened by many_begin_kernel.  xo / lo double as the kept last solution the warm starts read.
template <typename T>
class ManyHandleT : public ManyHandle {
 public:
  ManyHandleT(int ord, ManyShapes<T> &&shapes, const void *Ain, int mem, int device)
      : sh_(std::move(shapes)), k_(sh_.k) {
    const double t0 = wall_s();
    ctx_.init(device, 0);
    hipStream_t s = ctx_.stream;
    many_layout(a_, ord, sh_.m0, sh_.n0);   // ragged: every kernel replaces the shape fields by the problem's own
    const size_t kz = static_cast<size_t>(k_);
    const size_t rows = sh_.rows(0, kz), cols = sh_.cols(0, kz), len = rows + cols, ws_e = sh_.wss(0, kz);
    std::memset(&info_, 0, sizeof(info_));
    info_.k = k_; info_.dtype = sizeof(T) == 8 ? POGS_AMD_F64 : POGS_AMD_F32; info_.m = sh_.m0; info_.n = sh_.n0;
    info_.resident_bytes = ManySet<T>::resident_bytes(kz, len, ws_e, sh_.ragged);
    try {
      set_.reserve(kz, rows, cols, ws_e, sh_.ragged, true);
    } catch (const std::exception &e) {
      (void)hipGetLastError();
      char buf[512], shape[96];
      many_shape_text(shape, sizeof(shape), sh_);
      std::snprintf(buf, sizeof(buf),
                    "many-problem handle: the resident footprint of %d problems of %s (%.1f MB) cannot be "
                    "allocated; PogsAmdSolveManyFn solves them in chunks [%s]",
                    k_, shape, static_cast<double>(info_.resident_bytes) / (1 << 20), e.what());
      throw Error(buf);
    }
    set_.wire(a_);
    if (sh_.ragged) {
      // the handle's table counts every offset from problem 0: the pools' base pointers are the handle's buffers
      std::vector<ManyProb<T>> tab;
      sh_.table(tab, 0, kz, 0);
      POGS_HIP_CHECK(hipMemcpyAsync(set_.prob.p, tab.data(), kz * sizeof(ManyProb<T>), hipMemcpyHostToDevice, s));
      POGS_HIP_CHECK(hipStreamSynchronize(s));
    }
    // setup in chunks: a host A through a staging buffer under the workspace cap; a chunk is also the y extent of
    // the copy and Gram grids
    const size_t cap = mem == POGS_AMD_HOST ? workspace_cap_bytes(ctx_.device) : ~static_cast<size_t>(0);
    const std::vector<size_t> starts = many_chunks(kz, cap, 32768, [&](size_t j) {
      return mem == POGS_AMD_HOST ? sh_.els(j, 1) * sizeof(T) : static_cast<size_t>(0);
    });
    const ManyStage<T> stage(sh_, Ain, mem, starts);
    const DevBuf<T> rnd = many_start_vector<T>(sh_.n0, s);
    for (size_t ci = 0; ci + 1 < starts.size(); ++ci) {
      const size_t j0 = starts[ci];
      const int cnt = static_cast<int>(starts[ci + 1] - j0);
      // the chunk's problems are q = 0 .. cnt - 1 of this launch.  Uniform: the bases move to the chunk.  Ragged: the
      // table rows move, their offsets still count from problem 0, so ws stays, and src0 says that src points at the
      // chunk's first matrix
      ManyArgs<T> c = a_;
      c.st += j0;
      c.rnd = rnd.p;
      c.src = stage.chunk(j0, cnt, s);
      if (sh_.ragged) {
        c.prob += j0;
        c.src0 = sh_.el0(j0);
      } else {
        c.ws += sh_.ws0(j0);
      }
      many_setup(c, cnt, many_extent(sh_, j0, cnt), set_.ws.p + sh_.ws0(j0), s);
    }
    ctx_.sync();
    ext_ = many_extent(sh_, 0, kz);
    last_status_.assign(kz, POGS_ERROR);
    last_rho_.assign(kz, 1.0);
    info_.setup_s = wall_s() - t0;
  }
  ~ManyHandleT() override { (void)hipStreamSynchronize(ctx_.stream); }

  int device() const override { return ctx_.device; }
  int count() const override { return k_; }
  PogsAmdManyInfo info() const override { return info_; }
  void shapes(size_t *m, size_t *n) const override {
    for (size_t j = 0; j < static_cast<size_t>(k_); ++j) {
      m[j] = sh_.m(j);
      n[j] = sh_.n(j);
    }
  }

  void solve(const FnHost *f, const FnHost *g, const ManyStart &sa, const SolveParams &p, const BatchOut &out) override {
    POGS_CHECK(out.x && out.final_iter && out.status, "many-problem handle: x, final_iter and status must not be NULL");
    POGS_CHECK(sa.start == POGS_AMD_MANY_COLD || sa.start == POGS_AMD_MANY_WARM_GIVEN ||
               sa.start == POGS_AMD_MANY_WARM_LAST, "many-problem handle: unknown start mode");
    POGS_CHECK(sa.start != POGS_AMD_MANY_WARM_GIVEN || (sa.x0 && sa.l0),
               "many-problem handle: a given warm start needs both x0 and l0 (pogs.cpp:159-179)");
    POGS_CHECK(sa.start != POGS_AMD_MANY_WARM_LAST || solved_,
               "many-problem handle: start = last before the handle's first solve");
    const double t0 = wall_s();
    hipStream_t s = ctx_.stream;
    const size_t kz = static_cast<size_t>(k_);
    hwarm_.resize(kz);
    rho_.resize(kz);
    for (size_t q = 0; q < kz; ++q) {
      const bool kept = last_status_[q] == POGS_SUCCESS || last_status_[q] == POGS_MAX_ITER;
      hwarm_[q] = sa.start == POGS_AMD_MANY_WARM_GIVEN || (sa.start == POGS_AMD_MANY_WARM_LAST && kept);
      rho_[q] = sa.rho ? sa.rho[q] : 1.0;
      if (sa.start == POGS_AMD_MANY_WARM_LAST) rho_[q] = !kept ? 1.0 : sa.rho ? sa.rho[q] : last_rho_[q];
    }
    set_.open(f, g, sh_, 0, k_, p, rho_.data(), s);
    const int *warm = nullptr;
    if (sa.start != POGS_AMD_MANY_COLD) {
      POGS_HIP_CHECK(hipMemcpyAsync(set_.warm.p, hwarm_.data(), kz * sizeof(int), hipMemcpyHostToDevice, s));
      warm = set_.warm.p;
    }
    if (sa.start == POGS_AMD_MANY_WARM_GIVEN) {
      POGS_HIP_CHECK(hipMemcpyAsync(set_.xo.p, sa.x0, sh_.cols(0, kz) * sizeof(T), hipMemcpyHostToDevice, s));
      POGS_HIP_CHECK(hipMemcpyAsync(set_.lo.p, sa.l0, sh_.rows(0, kz) * sizeof(T), hipMemcpyHostToDevice, s));
    }
    ctx_.sync();
    const double t1 = wall_s();
    hipLaunchKernelGGL(many_begin_kernel<T>, dim3(k_), dim3(kTPB), 0, s, a_, warm);
    POGS_HIP_CHECK(hipGetLastError());
    const unsigned long long launches = 1 + many_run_loop(a_, k_, ext_, p.max_iter, set_.hdone.p, s);
    const double t_loop = wall_s() - t1;
    set_.fetch(sh_, 0, kz, out, s);
    // the control blocks come back for the rho every problem stopped at
    std::vector<AdmmControl<T>> &ch = set_.ch;
    POGS_HIP_CHECK(hipMemcpyAsync(ch.data(), set_.ctl.p, kz * sizeof(AdmmControl<T>), hipMemcpyDeviceToHost, s));
    POGS_HIP_CHECK(hipStreamSynchronize(s));
    unsigned long long piters = 0;
    for (size_t q = 0; q < kz; ++q) {
      last_status_[q] = out.status[q];
      last_rho_[q] = static_cast<double>(ch[q].rho);
      if (sa.rho_final) sa.rho_final[q] = last_rho_[q];
      piters += out.final_iter[q] + 1ull;
    }
    solved_ = true;
    info_.loop_s = t_loop;
    info_.launches = launches;
    info_.problem_iters = piters;
    if (p.verbose > 0) {
      static const char *const kStart[3] = {"cold", "warm (given)", "warm (last)"};
      char head[240], shape[96];
      many_shape_text(shape, sizeof(shape), sh_);
      std::snprintf(head, sizeof(head), "POGS-AMD many handle: %d %sproblems of %s (%s), start %s", k_,
                    sh_.ragged ? "ragged " : "", shape, sizeof(T) == 8 ? "fp64" : "fp32", kStart[sa.start]);
      many_print_summary(head, k_, out.final_iter, out.status, 0.0, t_loop, wall_s() - t0, launches);
    }
  }

 private:
  ManyShapes<T> sh_;
  int k_;
  Ctx ctx_;
  ManyArgs<T> a_{};
  ManyExtent ext_;
  ManySet<T> set_;                         // all k problems; xo / lo: the kept last solution
  std::vector<int> hwarm_, last_status_;   // each problem's status after the last solve (POGS_ERROR: none yet)
  std::vector<double> last_rho_, rho_;     // the rho it stopped at; the rho this solve starts it from
  bool solved_ = false;
  PogsAmdManyInfo info_;
};

}  // namespace

// The argument checks of every many-problem entry, `what` the prefix of their messages, in the order the entries
// report them: the call (dtype, k, ord, mem), then A and one shape's envelope.  A ragged entry checks its call the same
// way and words the rest per problem.
namespace {
void many_check_call(const std::string &what, int dtype, int ord, int k, int mem) {
  POGS_CHECK(dtype == POGS_AMD_F32 || dtype == POGS_AMD_F64, (what + ": unknown dtype").c_str());
  POGS_CHECK(k >= 1, (what + ": k must be >= 1").c_str());
  POGS_CHECK(ord == ROW_MAJ || ord == COL_MAJ, (what + ": unknown ord").c_str());
  POGS_CHECK(mem == POGS_AMD_HOST || mem == POGS_AMD_DEVICE, (what + ": unknown mem").c_str());
}

void many_check_uniform(const std::string &what, int dtype, int ord, int k, size_t m, size_t n, const void *A,
                        int mem) {
  many_check_call(what, dtype, ord, k, mem);
  POGS_CHECK(A != nullptr, (what + ": null A").c_str());
  POGS_CHECK(m >= 1 && n >= 1, (what + ": m and n must be >= 1").c_str());
  POGS_CHECK(std::min(m, n) <= POGS_AMD_MANY_MIN_DIM_MAX,
             (what + ": min(m, n) exceeds POGS_AMD_MANY_MIN_DIM_MAX").c_str());
  POGS_CHECK(std::max(m, n) <= POGS_AMD_MANY_MAX_DIM_MAX,
             (what + ": max(m, n) exceeds POGS_AMD_MANY_MAX_DIM_MAX").c_str());
}
}  // namespace

void many_check_args(int dtype, int ord, int k, size_t m, size_t n, const void *A, int mem) {
  many_check_uniform("many-problem solve", dtype, ord, k, m, n, A, mem);
}

void many_check_ragged(int dtype, int ord, int k, const size_t *m, const size_t *n, const void *A, int mem) {
  many_check_call("ragged many-problem solve", dtype, ord, k, mem);
  POGS_CHECK(m != nullptr && n != nullptr, "ragged many-problem solve: null m or n");
  POGS_CHECK(A != nullptr, "ragged many-problem solve: null A");
  for (int j = 0; j < k; ++j) {
    const char *why = m[j] < 1 || n[j] < 1 ? "m and n must be >= 1"
                      : std::min(m[j], n[j]) > POGS_AMD_MANY_MIN_DIM_MAX ? "min(m, n) exceeds POGS_AMD_MANY_MIN_DIM_MAX"
                      : std::max(m[j], n[j]) > POGS_AMD_MANY_MAX_DIM_MAX ? "max(m, n) exceeds POGS_AMD_MANY_MAX_DIM_MAX"
                                                                          : nullptr;
    if (why) {
      char buf[256];
      std::snprintf(buf, sizeof(buf), "ragged many-problem solve: problem %d of %d (m[%d] = %zu, n[%d] = %zu): %s", j, k,
                    j, m[j], j, n[j], why);
      throw Error(buf);
    }
  }
}

namespace {
// fn(T()) with T the arithmetic type of the call: the one place an entry's dtype turns into a template argument.
template <typename F>
auto many_dispatch(int dtype, F fn) {
  if (dtype == POGS_AMD_F64) return fn(double());
  return fn(float());
}

// What the solve and create entries are called with: k problems of m x n, or (ragged) of mv[j] x nv[j].
struct ManyCall {
  bool ragged;
  int dtype, ord, k;
  size_t m, n;
  const size_t *mv, *nv;
  const void *A;
  int mem;
  void check() const {
    if (ragged) many_check_ragged(dtype, ord, k, mv, nv, A, mem);
    else many_check_args(dtype, ord, k, m, n, A, mem);
  }
  template <typename T>
  ManyShapes<T> shapes() const {
    ManyShapes<T> sh;
    if (ragged) sh.set_ragged(k, mv, nv);
    else sh.set_uniform(k, m, n);
    return sh;
  }
};

ManyHandle *many_create_any(const ManyCall &c, int device) {
  c.check();
  DeviceGuard guard(device);
  return many_dispatch(c.dtype, [&](auto t) -> ManyHandle * {
    using T = decltype(t);
    return new ManyHandleT<T>(c.ord, c.shapes<T>(), c.A, c.mem, device);
  });
}

void solve_many_any(const ManyCall &c, int device, const FnHost *f, const FnHost *g, const double *rho,
                    const SolveParams &p, const BatchOut &out) {
  c.check();
  POGS_CHECK(out.x && out.final_iter && out.status,
             c.ragged ? "ragged many-problem solve: x, final_iter and status must not be NULL"
                      : "many-problem solve: x, final_iter and status must not be NULL");
  many_dispatch(c.dtype, [&](auto t) {
    using T = decltype(t);
    solve_many_t<T>(c.ord, c.shapes<T>(), c.A, c.mem, device, f, g, rho, p, out);
  });
}
}  // namespace

ManyHandle *many_create(int dtype, int ord, int k, size_t m, size_t n, const void *A, int mem, int device) {
  return many_create_any({false, dtype, ord, k, m, n, nullptr, nullptr, A, mem}, device);
}

ManyHandle *many_create_ragged(int dtype, int ord, int k, const size_t *m, const size_t *n, const void *A, int mem,
                               int device) {
  return many_create_any({true, dtype, ord, k, 0, 0, m, n, A, mem}, device);
}

void solve_many(int dtype, int ord, int k, size_t m, size_t n, const void *A, int mem, int device, const FnHost *f,
                const FnHost *g, const double *rho, const SolveParams &p, const BatchOut &out) {
  solve_many_any({false, dtype, ord, k, m, n, nullptr, nullptr, A, mem}, device, f, g, rho, p, out);
}

void solve_many_ragged(int dtype, int ord, int k, const size_t *m, const size_t *n, const void *A, int mem, int device,
                       const FnHost *f, const FnHost *g, const double *rho, const SolveParams &p, const BatchOut &out) {
  solve_many_any({true, dtype, ord, k, 0, 0, m, n, A, mem}, device, f, g, rho, p, out);
}

void many_setup_check(int dtype, int ord, int k, size_t m, size_t n, const void *A, int mem, void *A_eq, void *d,
                      void *e, double *nrmA, void *W) {
  many_check_uniform("many setup check", dtype, ord, k, m, n, A, mem);
  many_dispatch(dtype, [&](auto t) {
    using T = decltype(t);
    many_setup_check_t<T>(ord, k, m, n, A, mem, static_cast<T *>(A_eq), static_cast<T *>(d), static_cast<T *>(e), nrmA,
                          static_cast<T *>(W));
  });
}

}  // namespace pogs_amd

// The many-problem solves' arithmetic on shapes: a problem's workspace layout, the iterations of one
// loop launch, the packed arrays' prefix sums, the ragged table's rows and the packing of problems into chunks.  Plain
// C++ with no HIP header, so that a host program can include it and check the numbers (tests/test_many_plan_host.py);
// many_device.h and the driver in many_kernels.hip build on it.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

#if defined(__HIPCC__)
#define POGS_PLAN_HD __host__ __device__ __forceinline__
#else
#define POGS_PLAN_HD inline
#endif

namespace pogs_amd {

constexpr int kMaxIterPerLaunch = 64;
// Work of one workgroup in one launch is bounded by about this many bytes streamed (the Sinkhorn-Knopp passes, the
// power iterations and the ADMM iterations are cut into launches by it), so that no launch runs long at the edge of
// the envelope (16384 x 512 fp64 = 64 MB per pass over A).
constexpr double kLaunchBytes = 256.0 * (1 << 20);

// x-sized and y-sized work vectors of a problem (z = [x | y] of pogs.cpp:129-138, its copies, the scalings)
enum XVec : int { kX = 0, kXt, kXprev, kX12, kXtemp, kE, kXs, kNumX };
enum YVec : int { kY = 0, kYt, kYprev, kY12, kYtemp, kD, kYs, kNumY };

// A problem's shape and where its arrays start in its workspace: the leading members of the kernels' ManyArgs.
struct ManyLayout {
  int m, n, k, tall;
  size_t stride;                 // elements of T per problem in ws
  size_t oA, oW, oT, ox[kNumX], oy[kNumY];
};

// A problem's workspace layout from its shape alone (offsets in elements of T): every array starts on a multiple of
// 64 elements, and so does the next problem's workspace.
POGS_PLAN_HD void many_offsets(ManyLayout &a, int m, int n) {
  const int K = m < n ? m : n;
  const size_t mz = static_cast<size_t>(m), nz = static_cast<size_t>(n), Kz = static_cast<size_t>(K);
  const size_t rm = (mz + 63) / 64 * 64, rn = (nz + 63) / 64 * 64;
  a.m = m; a.n = n; a.k = K; a.tall = m > n;
  size_t off = 0;
  a.oA = off; off += (mz * nz + 63) / 64 * 64;
  a.oW = off; off += (Kz * Kz + 63) / 64 * 64;
  a.oT = off; off += (Kz + 63) / 64 * 64;
  for (int v = 0; v < kNumX; ++v) { a.ox[v] = off; off += rn; }
  for (int v = 0; v < kNumY; ++v) { a.oy[v] = off; off += rm; }
  a.stride = off;
}

// ADMM iterations per loop launch: kMaxIterPerLaunch, fewer where an iteration streams much (kLaunchBytes).
template <typename T>
int many_iters_per_launch(size_t mn, int K) {
  const double iter_bytes = (2.0 * static_cast<double>(mn) + static_cast<double>(K) * K) * sizeof(T);
  return static_cast<int>(std::max(1.0, std::min<double>(kMaxIterPerLaunch, kLaunchBytes / iter_bytes)));
}

// One row of the ragged table (ManyArgs::prob): problem q's own shape, where it lives in every pool (element
// offsets from the pools' base pointers in ManyArgs), its Sinkhorn-Knopp regularisers and its iteration bound.
template <typename T>
struct ManyProb {
  int m, n;
  int ipl, pad;                  // ADMM iterations per loop launch (many_iters_per_launch of its shape)
  size_t ws, src, xo, yo;        // workspace; staged input; x-sized outputs (x, mu); y-sized outputs (y, l)
  T ce, cd;
};

// The shapes of a call's k problems and where problem j starts in every packed array: rows (f, y, l), columns
// (g, x, mu), matrix elements (A) and workspace elements, as k + 1 prefix sums.  A uniform call stores its one shape k
// times; `ragged` says only that the kernels read the shapes from a table (table()) and that the messages say so.
template <typename T>
struct ManyShapes {
  int k = 0;
  bool ragged = false;
  size_t m0 = 0, n0 = 0;                       // the largest m and the largest n (uniform: the shape)
  std::vector<size_t> mv, nv, r0, c0, e0, w0;  // the shapes and the k + 1 prefix sums

  void set_uniform(int kk, size_t m, size_t n) {
    mv.assign(static_cast<size_t>(kk), m); nv.assign(static_cast<size_t>(kk), n);
    fill(kk, false);
  }
  void set_ragged(int kk, const size_t *m, const size_t *n) {
    mv.assign(m, m + kk); nv.assign(n, n + kk);
    fill(kk, true);
  }
  size_t m(size_t j) const { return mv[j]; }
  size_t n(size_t j) const { return nv[j]; }
  size_t row0(size_t j) const { return r0[j]; }
  size_t col0(size_t j) const { return c0[j]; }
  size_t el0(size_t j) const { return e0[j]; }
  size_t ws0(size_t j) const { return w0[j]; }
  // the extent of problems [j0, j0 + cnt) in each packed array
  size_t rows(size_t j0, size_t cnt) const { return r0[j0 + cnt] - r0[j0]; }
  size_t cols(size_t j0, size_t cnt) const { return c0[j0 + cnt] - c0[j0]; }
  size_t els(size_t j0, size_t cnt) const { return e0[j0 + cnt] - e0[j0]; }
  size_t wss(size_t j0, size_t cnt) const { return w0[j0 + cnt] - w0[j0]; }
  // the rows of the ragged table for problems [j0, j0 + cnt), offsets counted from problem `base`
  void table(std::vector<ManyProb<T>> &t, size_t j0, size_t cnt, size_t base) const {
    t.resize(cnt);
    for (size_t q = 0; q < cnt; ++q) {
      const size_t j = j0 + q, mj = mv[j], nj = nv[j];
      ManyProb<T> &p = t[q];
      p.m = static_cast<int>(mj); p.n = static_cast<int>(nj);
      p.ipl = many_iters_per_launch<T>(mj * nj, static_cast<int>(std::min(mj, nj)));
      p.pad = 0;
      p.ws = w0[j] - w0[base]; p.src = e0[j] - e0[base]; p.xo = c0[j] - c0[base]; p.yo = r0[j] - r0[base];
      p.ce = static_cast<T>(1e-4) * static_cast<T>(mj + nj) / static_cast<T>(mj);
      p.cd = static_cast<T>(1e-4) * static_cast<T>(mj + nj) / static_cast<T>(nj);
    }
  }

 private:
  void fill(int kk, bool is_ragged) {
    const size_t kz = static_cast<size_t>(kk);
    k = kk; ragged = is_ragged; m0 = 0; n0 = 0;
    r0.assign(kz + 1, 0); c0.assign(kz + 1, 0); e0.assign(kz + 1, 0); w0.assign(kz + 1, 0);
    for (size_t j = 0; j < kz; ++j) {
      ManyLayout a{};
      many_offsets(a, static_cast<int>(mv[j]), static_cast<int>(nv[j]));
      r0[j + 1] = r0[j] + mv[j]; c0[j + 1] = c0[j] + nv[j]; e0[j + 1] = e0[j] + mv[j] * nv[j];
      w0[j + 1] = w0[j] + a.stride;
      m0 = std::max(m0, mv[j]); n0 = std::max(n0, nv[j]);
    }
  }
};

// What the launches of problems [j0, j0 + cnt) are sized by: the largest matrix and the largest Gram order among
// them, the fewest and the most ADMM iterations per loop launch, and their workspace extent.
struct ManyExtent {
  size_t mn_max = 0, ws_elems = 0;
  int K_max = 0, ipl_min = kMaxIterPerLaunch, ipl_max = 1;
};
template <typename T>
ManyExtent many_extent(const ManyShapes<T> &sh, size_t j0, size_t cnt) {
  ManyExtent x;
  x.ws_elems = sh.wss(j0, cnt);
  for (size_t j = j0; j < j0 + cnt; ++j) {
    const size_t mn = sh.m(j) * sh.n(j);
    const int K = static_cast<int>(std::min(sh.m(j), sh.n(j)));
    const int ipl = many_iters_per_launch<T>(mn, K);
    x.mn_max = std::max(x.mn_max, mn);
    x.K_max = std::max(x.K_max, K);
    x.ipl_min = std::min(x.ipl_min, ipl);
    x.ipl_max = std::max(x.ipl_max, ipl);
  }
  return x;
}

// Problems packed into chunks in order: a chunk takes problems while their bytes (per(j)) fit under cap and their
// count under max_cnt, and holds at least one.  Returns the chunk starts and k.
template <typename Per>
std::vector<size_t> many_chunks(size_t k, size_t cap, size_t max_cnt, Per per) {
  std::vector<size_t> starts{0};
  size_t used = 0, cnt = 0;
  for (size_t j = 0; j < k; ++j) {
    const size_t b = per(j);
    if (cnt > 0 && (used + b > cap || cnt >= max_cnt)) {
      starts.push_back(j);
      used = 0;
      cnt = 0;
    }
    used += b;
    ++cnt;
  }
  starts.push_back(k);
  return starts;
}

}  // namespace pogs_amd

"""CPU test of the many-problem driver's arithmetic on shapes (pogs_amd/csrc/many_plan.h): the workspace layout, the
iterations per loop launch, the packing of problems into chunks, the prefix sums of ManyShapes, many_extent and the
ragged table's rows.  The header is plain C++, so a small program with its own main includes it, is compiled with the
system C++ compiler and checks the numbers; neither a GPU nor the library is needed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <vector>

#include "many_plan.h"

using namespace pogs_amd;

#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::printf("line %d: CHECK(%s) failed\n", __LINE__, #cond);       \
      std::exit(1);                                                      \
    }                                                                    \
  } while (0)

static ManyLayout layout(int m, int n) {
  ManyLayout a{};
  many_offsets(a, m, n);
  return a;
}

static void check_layout(int m, int n) {
  const ManyLayout a = layout(m, n);
  CHECK(a.m == m && a.n == n);
  CHECK(a.k == (m < n ? m : n));
  CHECK(a.tall == (m > n ? 1 : 0));
  // every array starts on a multiple of 64 elements, in order, without overlap, and the stride closes the last one
  std::vector<size_t> at = {a.oA, a.oW, a.oT};
  std::vector<size_t> len = {size_t(m) * n, size_t(a.k) * a.k, size_t(a.k)};
  for (int v = 0; v < kNumX; ++v) { at.push_back(a.ox[v]); len.push_back(n); }
  for (int v = 0; v < kNumY; ++v) { at.push_back(a.oy[v]); len.push_back(m); }
  at.push_back(a.stride);
  CHECK(at[0] == 0);
  for (size_t i = 0; i + 1 < at.size(); ++i) {
    CHECK(at[i] % 64 == 0);
    CHECK(at[i] + len[i] <= at[i + 1]);
    CHECK(at[i + 1] - at[i] < len[i] + 64);
  }
  CHECK(a.stride % 64 == 0);
}

static void check_chunks(const std::vector<size_t> &bytes, size_t cap, size_t max_cnt, const std::vector<size_t> &st) {
  const size_t k = bytes.size();
  CHECK(st.size() >= 2 && st.front() == 0 && st.back() == k);
  for (size_t c = 0; c + 1 < st.size(); ++c) {
    CHECK(st[c] < st[c + 1]);                       // in order, no gap, at least one problem
    const size_t cnt = st[c + 1] - st[c];
    size_t used = 0;
    for (size_t j = st[c]; j < st[c + 1]; ++j) used += bytes[j];
    CHECK(used <= cap || cnt == 1);
    CHECK(cnt <= max_cnt || cnt == 1);
  }
}

template <typename T>
static void check_starts(const ManyShapes<T> &sh, const std::vector<size_t> &m, const std::vector<size_t> &n) {
  const size_t k = m.size();
  CHECK(sh.k == static_cast<int>(k));
  size_t r = 0, c = 0, e = 0, w = 0, mmax = 0, nmax = 0;
  for (size_t j = 0; j <= k; ++j) {
    CHECK(sh.row0(j) == r && sh.col0(j) == c && sh.el0(j) == e && sh.ws0(j) == w);
    if (j == k) break;
    CHECK(sh.m(j) == m[j] && sh.n(j) == n[j]);
    CHECK(sh.rows(j, 1) == m[j] && sh.cols(j, 1) == n[j] && sh.els(j, 1) == m[j] * n[j]);
    CHECK(sh.wss(j, 1) == layout(static_cast<int>(m[j]), static_cast<int>(n[j])).stride);
    r += m[j]; c += n[j]; e += m[j] * n[j]; w += sh.wss(j, 1);
    mmax = std::max(mmax, m[j]); nmax = std::max(nmax, n[j]);
  }
  CHECK(sh.rows(0, k) == r && sh.cols(0, k) == c && sh.els(0, k) == e && sh.wss(0, k) == w);
  CHECK(sh.m0 == mmax && sh.n0 == nmax);
}

int main() {
  // ---- the workspace layout
  CHECK(layout(7, 3).stride == 1088);
  CHECK(layout(500, 300).stride == 246208);
  CHECK(layout(45, 45).tall == 0 && layout(45, 45).k == 45);
  CHECK(layout(46, 45).tall == 1 && layout(45, 46).tall == 0);
  const int dims[][2] = {{7, 3}, {3, 7}, {500, 300}, {45, 45}, {1, 1}, {64, 64}, {65, 64}, {1, 30}, {200, 1},
                         {16384, 512}, {512, 16384}, {129, 127}};
  for (const auto &d : dims) check_layout(d[0], d[1]);

  // ---- iterations per loop launch
  CHECK(kMaxIterPerLaunch == 64);
  CHECK(many_iters_per_launch<double>(size_t(500) * 300, 300) == 64);
  CHECK(many_iters_per_launch<double>(size_t(16384) * 512, 512) == 1);
  CHECK(many_iters_per_launch<float>(size_t(16384) * 512, 512) == 3);

  // ---- chunks
  const std::vector<size_t> five = {10, 10, 10, 25, 5};
  auto per5 = [&](size_t j) { return five[j]; };
  const size_t none = ~size_t(0);
  CHECK((many_chunks(5, 20, none, per5) == std::vector<size_t>{0, 2, 3, 4, 5}));
  CHECK((many_chunks(5, none, 2, per5) == std::vector<size_t>{0, 2, 4, 5}));
  CHECK((many_chunks(5, none, 1, per5) == std::vector<size_t>{0, 1, 2, 3, 4, 5}));
  std::mt19937 gen(12345);
  for (int trial = 0; trial < 200; ++trial) {
    const size_t k = 1 + gen() % 40;
    std::vector<size_t> bytes(k);
    for (size_t &b : bytes) b = gen() % 100;      // zero-byte problems too
    const size_t cap = 1 + gen() % 250;
    const size_t max_cnt = trial % 3 == 0 ? 1 + gen() % 8 : none;
    check_chunks(bytes, cap, max_cnt, many_chunks(k, cap, max_cnt, [&](size_t j) { return bytes[j]; }));
  }

  // ---- ManyShapes: one representation for both setters
  {
    ManyShapes<double> u;
    u.set_uniform(5, 7, 3);
    CHECK(!u.ragged);
    for (size_t j = 0; j <= 5; ++j)
      CHECK(u.row0(j) == 7 * j && u.col0(j) == 3 * j && u.el0(j) == 21 * j && u.ws0(j) == 1088 * j);
    check_starts(u, std::vector<size_t>(5, 7), std::vector<size_t>(5, 3));
    // the same shapes as a ragged list: the same starts, and only the flag differs
    const std::vector<size_t> m7(5, 7), n3(5, 3);
    ManyShapes<double> r;
    r.set_ragged(5, m7.data(), n3.data());
    CHECK(r.ragged);
    for (size_t j = 0; j <= 5; ++j)
      CHECK(r.row0(j) == u.row0(j) && r.col0(j) == u.col0(j) && r.el0(j) == u.el0(j) && r.ws0(j) == u.ws0(j));
    for (size_t j = 0; j < 5; ++j) CHECK(r.m(j) == u.m(j) && r.n(j) == u.n(j));
    CHECK(r.m0 == u.m0 && r.n0 == u.n0 && u.m0 == 7 && u.n0 == 3);
  }
  {
    const std::vector<size_t> m = {40, 20, 33, 1, 200}, n = {20, 40, 7, 30, 1};
    ManyShapes<float> sh;
    sh.set_ragged(5, m.data(), n.data());
    CHECK(sh.ragged);
    check_starts(sh, m, n);
    // a setter replaces what an earlier one left
    sh.set_uniform(3, 9, 4);
    check_starts(sh, std::vector<size_t>(3, 9), std::vector<size_t>(3, 4));
    sh.set_ragged(5, m.data(), n.data());
    check_starts(sh, m, n);
    // table(): rows of problems [j0, j0 + cnt), every offset counted from problem `base`
    for (size_t base : {size_t(0), size_t(2)}) {
      std::vector<ManyProb<float>> t;
      sh.table(t, 2, 3, base);
      CHECK(t.size() == 3);
      for (size_t q = 0; q < 3; ++q) {
        const size_t j = 2 + q;
        CHECK(t[q].m == static_cast<int>(m[j]) && t[q].n == static_cast<int>(n[j]) && t[q].pad == 0);
        CHECK(t[q].ipl == many_iters_per_launch<float>(m[j] * n[j], static_cast<int>(std::min(m[j], n[j]))));
        CHECK(t[q].ws == sh.ws0(j) - sh.ws0(base) && t[q].src == sh.el0(j) - sh.el0(base));
        CHECK(t[q].xo == sh.col0(j) - sh.col0(base) && t[q].yo == sh.row0(j) - sh.row0(base));
        CHECK(t[q].ce == 1e-4f * static_cast<float>(m[j] + n[j]) / static_cast<float>(m[j]));
        CHECK(t[q].cd == 1e-4f * static_cast<float>(m[j] + n[j]) / static_cast<float>(n[j]));
      }
      if (base == 2) CHECK(t[0].ws == 0 && t[0].src == 0 && t[0].xo == 0 && t[0].yo == 0);
    }
    // many_extent of a sub-range looks at exactly its problems
    const ManyExtent x = many_extent(sh, 1, 3);      // (20, 40), (33, 7), (1, 30)
    CHECK(x.mn_max == 800 && x.K_max == 20 && x.ipl_min == 64 && x.ipl_max == 64);
    CHECK(x.ws_elems == sh.wss(1, 3));
    const ManyExtent y = many_extent(sh, 4, 1);      // (200, 1)
    CHECK(y.mn_max == 200 && y.K_max == 1 && y.ws_elems == sh.wss(4, 1));
  }
  {
    // shapes at which the iterations per launch differ (fp64: 1, 64, 3, 64)
    const std::vector<size_t> m = {16384, 500, 8192, 7}, n = {512, 300, 512, 3};
    ManyShapes<double> sh;
    sh.set_ragged(4, m.data(), n.data());
    const ManyExtent all = many_extent(sh, 0, 4);
    CHECK(all.mn_max == size_t(16384) * 512 && all.K_max == 512 && all.ipl_min == 1 && all.ipl_max == 64);
    const ManyExtent mid = many_extent(sh, 1, 2);
    CHECK(mid.mn_max == size_t(8192) * 512 && mid.K_max == 512 && mid.ipl_min == 3 && mid.ipl_max == 64);
    const ManyExtent one = many_extent(sh, 0, 1);
    CHECK(one.ipl_min == 1 && one.ipl_max == 1 && one.ws_elems == sh.ws0(1));
    const ManyExtent two = many_extent(sh, 2, 1);
    CHECK(two.ipl_min == 3 && two.ipl_max == 3 && two.K_max == 512);
    const ManyExtent last = many_extent(sh, 3, 1);
    CHECK(last.mn_max == 21 && last.K_max == 3 && last.ipl_min == 64 && last.ipl_max == 64 && last.ws_elems == 1088);
    // a uniform call's extent is its one shape's, whatever the sub-range
    ManyShapes<double> u;
    u.set_uniform(6, 500, 300);
    const ManyExtent ux = many_extent(u, 2, 3);
    CHECK(ux.mn_max == 150000 && ux.K_max == 300 && ux.ipl_min == 64 && ux.ipl_max == 64);
    CHECK(ux.ws_elems == size_t(3) * 246208);
  }
  std::printf("many_plan.h: all checks passed\n");
  return 0;
}
"""


def test_plan_arithmetic_in_a_host_program(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler on PATH")
    src = tmp_path / "many_plan_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "many_plan_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "pogs_amd", "csrc"), str(src),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout

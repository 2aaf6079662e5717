#pragma once
// Mixed storage (POGS_AMD_STORE_F32 on an fp64 handle): the one-pass iteration's pass over a `float` copy of the
// stored matrix with fp64 arithmetic.  The iteration of an fp64 handle is one HBM-bound pass over A; the iterates,
// sums, prox and residuals need 53 bits, the matrix entries -- data -- do not, so the handle rounds the equilibrated
// matrix to float ONCE (dense_setup.h: equilibrate), keeps both copies with EQUAL values (A_ in doubles, A32_ in
// floats) and lets the hot launches of step (D) of DenseSolver::iteration_fused read the narrow one: 4 instead of 8
// bytes per entry.  Every other pass keeps its fp64 kernel on A_; both copies hold the same numbers, so any mixture of
// the two is the same mathematics and only the order of some sums differs.
//
// stream_rows2_mixed_kernel has the contract of stream_rows2_kernel<double, ...> (stream.h): the same Op interface
// (Pre, prefetch, the row call, NS scalar sums), the same logical workgroup id, column partials [grid][n_pad] in
// DOUBLES, scalar partials [grid][NS], one fixed order of every sum.  FusedIterOp<double, false / true> (ops.h) is used
// unchanged.  The kernel lives in ONE translation unit (dense_mixed.hip) behind the non-template launch functions
// below: the per-shape objects (dense_plan.hip) gain a call, not a kernel.
//
// Where this kernel can go wrong, and what it does about it:
//   * VECTOR LENGTH.  Every x-side vector of an fp64 handle has n_pad = round_up(n, 2) elements; the float rows run to
//     n32 = round_up(n, 4).  When n_pad % 4 == 2 the last float vector of a row covers two columns for which NO x entry
//     and NO column-partial slot exists.  A float vector is therefore handled as two pairs of doubles (columns c, c + 1
//     and c + 2, c + 3): the upper pair's x entries are loaded, and its partials stored, only where c + 2 < n_pad, and
//     read as zero otherwise (the matrix's own padding columns are zero as well).  An out-of-bounds load is a GPU fault,
//     not a wrong digit.
//   * ROWS >= m IN THE LAST STEP.  Tile loads are unconditional, with row and column clamped into the matrix (the
//     unconditional-load lesson of the prefetching kernel, stream.h); the tile of a row past m is then zeroed by a mask,
//     not merely its u, and a lane past the row's end has zero x entries and stores no partials.
//   * THE FUNCTOR runs on the t < R lanes between two barriers; op.prefetch is issued ahead of the reduction, as in
//     stream_rows2_kernel.
//   * GRIDS.  The grid may exceed the number of row blocks: an idle workgroup still writes zero column partials and
//     zero scalar partials, as the second stage adds [grid] records.
//
// The second half of this file is the same idea for the one-pass CGLS projector (POGS_AMD_PROJ_CGLS_FUSED with
// POGS_AMD_STORE_F32, any shape: PogsAmdCreateDenseMixed): stream_rows_mixed_kernel, the single-vector pass in the
// three forms the device-resident loop launches, in its own translation unit (stream_mixed.hip).
#include <hip/hip_runtime.h>

#include "common.h"
#include "ops.h"
#include "reduce.h"
#include "stream.h"
#include "vec_kernels.h"

namespace pogs_amd {

struct StreamArgsMixed {
  const float *A;            // row-major, rows of n32 floats at stride lda (a multiple of 4), columns n .. n32 zero
  size_t lda;
  int m;
  int n_pad;                 // round_up(n, 2): length of the dot vectors and of a column-partial record
  int n32;                   // round_up(n, 4): floats of a row that are read
  const double *xin0, *xin1; // ND dot vectors (n_pad doubles each)
  double *col_partials0, *col_partials1;   // NA accumulators: [grid][n_pad] each
  double *scalar_partials;   // [grid][Op::NS]
};

// The mixed launch has its own plan: the shape make_stream_plan<float> chooses for rows of n32 floats.  The one-pass
// shapes of the mixed plan are the 64- and 256-thread ones: rows of up to 10240 columns, which is exactly where the
// one-pass iteration of an fp64 handle ends (stream2_supported on its own plan: 512 x 10 vectors of two doubles), so a
// wider shape could never be reached by a solve.  Windowed rows and wider shapes are refused at create.
struct MixedPlan {
  int tpb = 0, nv = 0;   // threads per workgroup, float4 vectors per thread and row
  int num_cu = 0;
  bool ok = false;
};
inline bool mixed_shape_listed(int tpb, int nv) {
#define POGS_MIXED_LISTED(TPB_, NV_) if (TPB_ <= 256 && tpb == TPB_ && nv == NV_) return true;
  POGS_STREAM_PLANS(POGS_MIXED_LISTED)
#undef POGS_MIXED_LISTED
  return false;
}
inline MixedPlan mixed_plan_of_shape(int tpb, int nv, int num_cu) {
  MixedPlan p;
  p.tpb = tpb; p.nv = nv; p.num_cu = num_cu;
  p.ok = mixed_shape_listed(tpb, nv);
  return p;
}
inline MixedPlan make_mixed_plan(size_t n, int num_cu) {
  const StreamPlan f = make_stream_plan<float>(static_cast<int>(round_up(n, 4)), num_cu);
  if (!f.ok || f.xl) return MixedPlan{};
  return mixed_plan_of_shape(f.tpb, f.nv, num_cu);
}

// Rows per step and workgroups per CU, from the register budget.  Per thread the kernel holds, in 32-bit registers,
//   the tile 4 NV R (floats)  +  the first dot vector 8 NV (doubles)  +  NA accumulators 8 NV each  +  ~100
// (functor operands, the logistic prox, six scalar sums, addresses; what the compiler reports for the instances built
// lies within a few registers of this: all within 256, one -- the full logistic form at 512 x 5 -- with five registers
// of scratch); the second dot vector sits in LDS.  A CU has 4 SIMDs with 512 registers per lane each: B workgroups of
// 256 threads per CU leave a wavefront 512 / B.  Of B = 3 (168 registers) and B = 2 (256) the one with more rows in
// flight per CU wins, three on a tie (more workgroups hide the row functor).  64-thread workgroups run eight per CU and
// 512-thread ones one (two wavefronts per SIMD, 256 registers, both).
//
// THE EXECUTION SHAPE.  With doubles for x and the accumulators a thread of a 256 x 6 .. 10 shape (24 .. 40 columns) needs
// more than 256 registers; the compiler then parks the tile in the accumulation half of the file and copies every entry
// in and out (measured at 256 x 10, one workgroup per CU: 0.61 x the fp64 handle's rate).  Those shapes therefore RUN
// with 512 threads and half the vectors per thread -- the same columns, 12 .. 20 per thread, the column split of the
// fp64 plan's 512 x 6 .. 10 -- one workgroup per CU, two wavefronts per SIMD, 256 registers each.  The plan (and info,
// force_tpb / force_nv) keep naming the shape of POGS_STREAM_PLANS.
constexpr int mixed_exec_tpb(int tpb, int nv) { return (tpb == 256 && nv >= 6) ? 512 : tpb; }
constexpr int mixed_exec_nv(int tpb, int nv) { return (tpb == 256 && nv >= 6) ? nv / 2 : nv; }
constexpr int mixed_regs_est(int nv, int r, int na) { return 4 * nv * r + 8 * nv * (1 + na) + 100; }
constexpr int mixed_rows_fit(int nv, int na, int budget) {
  return mixed_regs_est(nv, 8, na) <= budget ? 8 : mixed_regs_est(nv, 4, na) <= budget ? 4 : mixed_regs_est(nv, 3, na) <= budget ? 3
         : mixed_regs_est(nv, 2, na) <= budget ? 2 : mixed_regs_est(nv, 1, na) <= budget ? 1 : 0;
}
// (the three functions below take the EXECUTION shape)
constexpr int mixed_blocks_per_cu(int tpb, int nv, int na) {
  if (tpb == 512) return 1;
  if (tpb != 256) return 8;
  const int r3 = 3 * mixed_rows_fit(nv, na, 168), r2 = 2 * mixed_rows_fit(nv, na, 256);
  return (r3 >= r2 && r3 > 0) ? 3 : 2;
}
constexpr int mixed_rows_c(int tpb, int nv, int na) {
  return mixed_rows_fit(nv, na, (tpb == 256 && mixed_blocks_per_cu(tpb, nv, na) == 3) ? 168 : 256);
}
constexpr int mixed_waves_per_simd(int tpb, int nv, int na) {
  return (mixed_blocks_per_cu(tpb, nv, na) * (tpb / 64) + 3) / 4;
}
// (full = two dots and two accumulators, else the lean form: one and one)
inline int mixed_rows(const MixedPlan &p, bool full) {
  return mixed_rows_c(mixed_exec_tpb(p.tpb, p.nv), mixed_exec_nv(p.tpb, p.nv), full ? 2 : 1);
}
inline int mixed_grid_cap(const MixedPlan &p, bool full) {
  return p.num_cu * mixed_blocks_per_cu(mixed_exec_tpb(p.tpb, p.nv), mixed_exec_nv(p.tpb, p.nv), full ? 2 : 1);
}
inline int mixed_grid_max(const MixedPlan &p) { return std::max(mixed_grid_cap(p, false), mixed_grid_cap(p, true)); }
inline int mixed_grid(const MixedPlan &p, bool full, int m) {
  const int R = mixed_rows(p, full), nblk = (m + R - 1) / R, gmax = mixed_grid_cap(p, full);
  return nblk < gmax ? (nblk > 0 ? nblk : 1) : gmax;
}

// The launches (dense_mixed.hip).  full: two dots (xin0, xin1) and two accumulators; else one and one.
void launch_stream2_mixed(const MixedPlan &p, bool full, const StreamArgsMixed &a, const FusedIterOp<double, false> &op,
                          hipStream_t s);
void launch_stream2_mixed(const MixedPlan &p, bool full, const StreamArgsMixed &a, const FusedIterOp<double, true> &op,
                          hipStream_t s);
// A32[i][j] = (float)A[i][j];  A[i][j] = (double)A32[i][j]   (columns n .. n32 of A32 written as zero)
void launch_round_to_f32(double *A, size_t lda, float *A32, size_t lda32, int m, int n, int grid, hipStream_t s);

template <int TPB, int NV, int R, int ND, int NA, typename Op>
__global__ void __launch_bounds__(TPB, mixed_waves_per_simd(TPB, NV, NA)) stream_rows2_mixed_kernel(StreamArgsMixed a, Op op) {
  static_assert((ND == 1 && NA == 1) || (ND == 2 && NA == 2), "the lean and the full form");
  static_assert(R >= 1 && R <= 64, "the row functor runs on the lanes t < R of the first wavefront");
  constexpr int NW = TPB / 64;
  constexpr int NS = Op::NS > 0 ? Op::NS : 1;
  __shared__ double s_part[2 * R * ND * NW];
  __shared__ double s_u[2 * R * NA];
  __shared__ double s_red[NS * NW];
  const unsigned bid = dev::logical_block_id();
  // the second dot vector lives in LDS (dynamic, n32 doubles, zero past n_pad), as in stream_rows2_kernel
  extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];
  double *s_x1 = reinterpret_cast<double *>(s_dyn);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;

  // float vector v of this thread covers columns c .. c + 3, c = (v TPB + t) 4: the pair (c, c + 1) exists in the
  // x-side vectors whenever the vector is inside the row (c < n32 implies c < n <= n_pad), the pair (c + 2, c + 3) only
  // if c + 2 < n_pad -- not in the last vector of a row when n_pad % 4 == 2
  double2 xlo[NV], xhi[NV];
  double2 acc[NA][2 * NV];
  int colc[NV];   // the column a lane loads: its own, or (past n32) the row's last vector
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int c = (v * TPB + t) * 4;
    const bool lo = c < a.n32, hi = c + 2 < a.n_pad;
    colc[v] = lo ? c : a.n32 - 4;
    xlo[v] = lo ? *reinterpret_cast<const double2 *>(a.xin0 + c) : make_double2(0.0, 0.0);
    xhi[v] = hi ? *reinterpret_cast<const double2 *>(a.xin0 + c + 2) : make_double2(0.0, 0.0);
    if (ND > 1 && lo) {
      *reinterpret_cast<double2 *>(s_x1 + c) = *reinterpret_cast<const double2 *>(a.xin1 + c);
      *reinterpret_cast<double2 *>(s_x1 + c + 2) = hi ? *reinterpret_cast<const double2 *>(a.xin1 + c + 2) : make_double2(0.0, 0.0);
    }
  }
  if (ND > 1) __syncthreads();
#pragma unroll
  for (int q = 0; q < NA; ++q)
#pragma unroll
    for (int v = 0; v < 2 * NV; ++v) acc[q][v] = make_double2(0.0, 0.0);
  double sacc[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) sacc[k] = 0.0;

  const int nblk = (a.m + R - 1) / R;
  int slot = 0;
  for (int blk = bid; blk < nblk; blk += gridDim.x, slot ^= 1) {
    const int row0 = blk * R;
    // the tile stays in floats (half the registers of a tile of doubles); an entry is widened where it is used --
    // exactly, so the dots and the column sums see the same number
    // Every tile load is UNCONDITIONAL: row and column are clamped into the matrix (stream.h, the prefetching kernel's
    // lesson: a guarded load is a branch, and behind it the compiler waited for every load on its own -- measured here at
    // 256 x 10, 40 loads in turn per step: 2.2 TB/s).  A lane past n32 reads the row's last vector again: its x entries
    // are zero and its partials are never stored.  A row past m reads row m - 1 again and is then ZEROED (a mask, no
    // branch): the tile of such a row is zero, not merely its u.
    float4 av[R][NV];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int row = row0 + r;
      const float *rp = a.A + static_cast<size_t>(row < a.m ? row : a.m - 1) * a.lda;
      const unsigned keep = row < a.m ? 0xFFFFFFFFu : 0u;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        typedef unsigned int raw16 __attribute__((ext_vector_type(4)));
        const float4 val = stream_load<float4>(rp + colc[v]);
        raw16 bits;
        __builtin_memcpy(&bits, &val, 16);
        bits &= keep;
        __builtin_memcpy(&av[r][v], &bits, 16);
      }
    }
    // the row functor's own operands are requested now: their latency overlaps the tile's
    typename Op::Pre pre;
    if (t < R && row0 + t < a.m) pre = op.prefetch(row0 + t);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      double s0 = 0, s1 = 0;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        const double2 alo = make_double2(static_cast<double>(av[r][v].x), static_cast<double>(av[r][v].y));
        const double2 ahi = make_double2(static_cast<double>(av[r][v].z), static_cast<double>(av[r][v].w));
        s0 += dev::vdot(alo, xlo[v]);
        s0 += dev::vdot(ahi, xhi[v]);
        if (ND > 1) {
          const int c = (v * TPB + t) * 4;
          if (c < a.n32) {
            s1 += dev::vdot(alo, *reinterpret_cast<const double2 *>(s_x1 + c));
            s1 += dev::vdot(ahi, *reinterpret_cast<const double2 *>(s_x1 + c + 2));
          }
        }
      }
      s0 = dev::wave_sum(s0);
      if (ND > 1) s1 = dev::wave_sum(s1);
      if (lane == 0) {
        s_part[((slot * R + r) * ND + 0) * NW + wave] = s0;
        if (ND > 1) s_part[((slot * R + r) * ND + 1) * NW + wave] = s1;
      }
    }
    __syncthreads();
    if (t < R) {
      const int row = row0 + t;
      double uu[NA];
#pragma unroll
      for (int q = 0; q < NA; ++q) uu[q] = 0;
      if (row < a.m) {
        double dots[ND];
#pragma unroll
        for (int d = 0; d < ND; ++d) {
          double s = 0;
#pragma unroll
          for (int w = 0; w < NW; ++w) s += s_part[((slot * R + t) * ND + d) * NW + w];
          dots[d] = s;
        }
        op.row(row, pre, dots, sacc, uu);
      }
#pragma unroll
      for (int q = 0; q < NA; ++q) s_u[(slot * R + t) * NA + q] = uu[q];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r) {
      double uu[NA];
#pragma unroll
      for (int q = 0; q < NA; ++q) uu[q] = s_u[(slot * R + r) * NA + q];
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        // (the floats are made opaque here: otherwise the compiler keeps the doubles of the dot phase alive across the
        //  functor instead of widening again, and the tile takes the registers of a tile of doubles after all)
        asm volatile("" : "+v"(av[r][v].x), "+v"(av[r][v].y), "+v"(av[r][v].z), "+v"(av[r][v].w));
        const double2 alo = make_double2(static_cast<double>(av[r][v].x), static_cast<double>(av[r][v].y));
        const double2 ahi = make_double2(static_cast<double>(av[r][v].z), static_cast<double>(av[r][v].w));
#pragma unroll
        for (int q = 0; q < NA; ++q) {
          dev::vfma(acc[q][2 * v], uu[q], alo);
          dev::vfma(acc[q][2 * v + 1], uu[q], ahi);
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < NA; ++q) {
    double *out = (q == 0 ? a.col_partials0 : a.col_partials1) + static_cast<size_t>(bid) * a.n_pad;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int c = (v * TPB + t) * 4;
      if (c < a.n32) *reinterpret_cast<double2 *>(out + c) = acc[q][2 * v];
      if (c + 2 < a.n_pad) *reinterpret_cast<double2 *>(out + c + 2) = acc[q][2 * v + 1];
    }
  }
  if (Op::NS > 0) {
    __syncthreads();
    dev::block_sum<NS, TPB>(sacc, s_red);
    if (t == 0) {
#pragma unroll
      for (int k = 0; k < NS; ++k) a.scalar_partials[static_cast<size_t>(bid) * NS + k] = sacc[k];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// stream_rows_mixed_kernel: the SINGLE-VECTOR streaming pass over the float copy, for the one-pass CGLS projector of a
// mixed-storage handle (dense_cg_fused.h).  The contract of stream_rows_kernel<double, ...> (stream.h) over a float
// matrix: the same Op interface (row(i, dot, s) returns the row's coefficient, u(i) for the ACC-only form, NS scalar
// sums, kGuarded / skip() through StreamOpGuarded), column partials [grid][n_pad] in DOUBLES, scalar partials
// [grid][NS], one fixed order of every sum, no atomics.  Rows, the column-partial slot and the scalar-partial slot go
// by the logical workgroup id of the one-pass kernels (stream.h: a bijection, so every sum is what blockIdx.x gives).
// The tile handling is stream_rows2_mixed_kernel's: float4 non-temporal loads, unconditional on clamped rows and
// columns; the tile stays in floats and is widened where it is used; a float vector is two pairs of doubles, the upper
// pair present only where c + 2 < n_pad; a row past m is zeroed by a mask.  Three forms:
//   ACC       u = A^T r at the start of every projection            GemvTOp<double>    (no x vector, no barrier)
//   DOT + ACC L1 of every CG step: q = A p, |q|^2, t = A^T q         DcgQRowOp<double>  (guarded)
//   DOT       y = A x of the y-sync projection                       ProjTailOp<double> (no accumulators, one barrier)
// A guarded launch that finds the loop ended returns before any load or store.  An idle workgroup (grid larger than
// the number of row blocks) writes zero column partials and zero scalar partials.
// ---------------------------------------------------------------------------------------------------------------------

// L1's row functor of the device-resident CGLS loop (dense_cg_fused.h): q_i = dot, |q|^2, and q_i back as the
// coefficient of row i in the column sums t = A^T q.  It lives here, outside the per-shape objects' unnamed namespace,
// because the launch functions below name it.
template <typename T>
struct DcgQRowOp {
  static constexpr int NS = 1;
  static constexpr bool kGuarded = true;
  T *q;
  const double *S;
  __device__ __forceinline__ bool skip() const { return S[kFcDone] != 0.0; }
  template <int N>
  __device__ __forceinline__ T row(int i, T dot, double (&s)[N]) const {
    q[i] = dot;
    dev::prod_acc(s[0], dot, dot);
    return dot;
  }
  __device__ __forceinline__ T u(int) const { return 0; }
};

struct StreamArgsMixed1 {
  const float *A;            // as StreamArgsMixed::A
  size_t lda;
  int m;
  int n_pad, n32;            // round_up(n, 2), round_up(n, 4)
  const double *xin;         // DOT: n_pad doubles
  double *col_partials;      // ACC: [grid][n_pad]
  double *scalar_partials;   // Op::NS > 0: [grid][Op::NS]
};

// Rows per step and workgroups per CU, as for the one-pass kernel above.  Per thread, in 32-bit registers:
//   the tile 4 NV R (floats)  +  the x vector 8 NV (DOT)  +  the accumulators 8 NV (ACC)  +  ~40
// (addresses, the widened entries of the row at hand, one or two scalar sums, a cheap functor: no prox).  DOT-only
// holds no accumulators and ACC-only no x vector, so they take more rows per step at the same budget.  What the
// compiler reports for every instance is in DESIGN.md section 3.10; none uses scratch.
constexpr int mixed1_regs_est(int nv, int r, bool dot, bool acc) { return 4 * nv * r + 8 * nv * ((dot ? 1 : 0) + (acc ? 1 : 0)) + 40; }
constexpr int mixed1_rows_fit(int nv, bool dot, bool acc, int budget) {
  return mixed1_regs_est(nv, 8, dot, acc) <= budget ? 8 : mixed1_regs_est(nv, 4, dot, acc) <= budget ? 4
         : mixed1_regs_est(nv, 3, dot, acc) <= budget ? 3 : mixed1_regs_est(nv, 2, dot, acc) <= budget ? 2
         : mixed1_regs_est(nv, 1, dot, acc) <= budget ? 1 : 0;
}
// (the three functions below take the EXECUTION shape, mixed_exec_tpb / mixed_exec_nv)
constexpr int mixed1_blocks_per_cu(int tpb, int nv, bool dot, bool acc) {
  if (tpb == 512) return 1;
  if (tpb != 256) return 8;
  const int r3 = 3 * mixed1_rows_fit(nv, dot, acc, 168), r2 = 2 * mixed1_rows_fit(nv, dot, acc, 256);
  return (r3 >= r2 && r3 > 0) ? 3 : 2;
}
constexpr int mixed1_rows_c(int tpb, int nv, bool dot, bool acc) {
  return mixed1_rows_fit(nv, dot, acc, (tpb == 256 && mixed1_blocks_per_cu(tpb, nv, dot, acc) == 3) ? 168 : 256);
}
constexpr int mixed1_waves_per_simd(int tpb, int nv, bool dot, bool acc) {
  return (mixed1_blocks_per_cu(tpb, nv, dot, acc) * (tpb / 64) + 3) / 4;
}
inline int mixed1_rows(const MixedPlan &p, bool dot, bool acc) {
  return mixed1_rows_c(mixed_exec_tpb(p.tpb, p.nv), mixed_exec_nv(p.tpb, p.nv), dot, acc);
}
inline int mixed1_grid_cap(const MixedPlan &p, bool dot, bool acc) {
  return p.num_cu * mixed1_blocks_per_cu(mixed_exec_tpb(p.tpb, p.nv), mixed_exec_nv(p.tpb, p.nv), dot, acc);
}
inline int mixed1_grid_max(const MixedPlan &p) {
  return std::max(mixed1_grid_cap(p, false, true), std::max(mixed1_grid_cap(p, true, true), mixed1_grid_cap(p, true, false)));
}
inline int mixed1_grid(const MixedPlan &p, bool dot, bool acc, int m) {
  const int R = mixed1_rows(p, dot, acc), nblk = (m + R - 1) / R, gmax = mixed1_grid_cap(p, dot, acc);
  return nblk < gmax ? (nblk > 0 ? nblk : 1) : gmax;
}

// The launches (stream_mixed.hip); the functor's type names the form.
void launch_stream_mixed(const MixedPlan &p, const StreamArgsMixed1 &a, const GemvTOp<double> &op, hipStream_t s);     // ACC
void launch_stream_mixed(const MixedPlan &p, const StreamArgsMixed1 &a, const DcgQRowOp<double> &op, hipStream_t s);   // DOT + ACC
void launch_stream_mixed(const MixedPlan &p, const StreamArgsMixed1 &a, const ProjTailOp<double> &op, hipStream_t s);  // DOT

template <int TPB, int NV, int R, bool DOT, bool ACC, typename Op>
__global__ void __launch_bounds__(TPB, mixed1_waves_per_simd(TPB, NV, DOT, ACC)) stream_rows_mixed_kernel(StreamArgsMixed1 a, Op op) {
  static_assert(DOT || ACC, "a pass forms row dots, column sums or both");
  static_assert(R >= 1 && R <= 64, "the row functor runs on the lanes t < R of the first wavefront");
  if constexpr (StreamOpGuarded<Op>::value) {
    if (op.skip()) return;
  }
  constexpr int NW = TPB / 64;
  constexpr int NS = Op::NS > 0 ? Op::NS : 1;
  constexpr int NX = DOT ? NV : 1, NACC = ACC ? 2 * NV : 1;
  __shared__ double s_part[2 * R * NW];
  __shared__ double s_u[2 * R];
  __shared__ double s_red[NS * NW];
  const unsigned bid = dev::logical_block_id();
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;

  // float vector v of this thread covers columns c .. c + 3, c = (v TPB + t) 4: the pair (c, c + 1) exists in the
  // x-side vectors whenever c < n32, the pair (c + 2, c + 3) only if c + 2 < n_pad (stream_rows2_mixed_kernel)
  double2 xlo[NX], xhi[NX];
  double2 acc[NACC];
  int colc[NV];   // the column a lane loads: its own, or (past n32) the row's last vector
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int c = (v * TPB + t) * 4;
    const bool lo = c < a.n32, hi = c + 2 < a.n_pad;
    colc[v] = lo ? c : a.n32 - 4;
    if (DOT) {
      xlo[v] = lo ? *reinterpret_cast<const double2 *>(a.xin + c) : make_double2(0.0, 0.0);
      xhi[v] = hi ? *reinterpret_cast<const double2 *>(a.xin + c + 2) : make_double2(0.0, 0.0);
    }
  }
  if (ACC) {
#pragma unroll
    for (int v = 0; v < 2 * NV; ++v) acc[v] = make_double2(0.0, 0.0);
  }
  double sacc[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) sacc[k] = 0.0;

  const int nblk = (a.m + R - 1) / R;
  int slot = 0;
  for (int blk = bid; blk < nblk; blk += gridDim.x, slot ^= 1) {
    const int row0 = blk * R;
    // every tile load unconditional: row and column clamped into the matrix, a row past m zeroed by a mask; a lane past
    // n32 reads the row's last vector again -- its x entries are zero and its partials are never stored
    float4 av[R][NV];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int row = row0 + r;
      const float *rp = a.A + static_cast<size_t>(row < a.m ? row : a.m - 1) * a.lda;
      const unsigned keep = row < a.m ? 0xFFFFFFFFu : 0u;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        typedef unsigned int raw16 __attribute__((ext_vector_type(4)));
        const float4 val = stream_load<float4>(rp + colc[v]);
        raw16 bits;
        __builtin_memcpy(&bits, &val, 16);
        bits &= keep;
        __builtin_memcpy(&av[r][v], &bits, 16);
      }
    }
    if (DOT) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        double s0 = 0;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
          const double2 alo = make_double2(static_cast<double>(av[r][v].x), static_cast<double>(av[r][v].y));
          const double2 ahi = make_double2(static_cast<double>(av[r][v].z), static_cast<double>(av[r][v].w));
          s0 += dev::vdot(alo, xlo[v]);
          s0 += dev::vdot(ahi, xhi[v]);
        }
        s0 = dev::wave_sum(s0);
        if (lane == 0) s_part[(slot * R + r) * NW + wave] = s0;
      }
      __syncthreads();
      if (t < R) {
        const int row = row0 + t;
        double uval = 0;
        if (row < a.m) {
          double dot = 0;
#pragma unroll
          for (int w = 0; w < NW; ++w) dot += s_part[(slot * R + t) * NW + w];
          uval = op.row(row, dot, sacc);
        }
        if (ACC) s_u[slot * R + t] = uval;
      }
      if (ACC) __syncthreads();
    }
    if (ACC) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        double u;
        if (DOT) {
          u = s_u[slot * R + r];
        } else {
          u = (row0 + r < a.m) ? op.u(row0 + r) : 0.0;
        }
#pragma unroll
        for (int v = 0; v < NV; ++v) {
          // (opaque floats: the doubles of the dot phase are not kept alive across the functor, stream_rows2_mixed_kernel)
          if (DOT) asm volatile("" : "+v"(av[r][v].x), "+v"(av[r][v].y), "+v"(av[r][v].z), "+v"(av[r][v].w));
          const double2 alo = make_double2(static_cast<double>(av[r][v].x), static_cast<double>(av[r][v].y));
          const double2 ahi = make_double2(static_cast<double>(av[r][v].z), static_cast<double>(av[r][v].w));
          dev::vfma(acc[2 * v], u, alo);
          dev::vfma(acc[2 * v + 1], u, ahi);
        }
      }
    }
  }
  if (ACC) {
    double *out = a.col_partials + static_cast<size_t>(bid) * a.n_pad;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int c = (v * TPB + t) * 4;
      if (c < a.n32) *reinterpret_cast<double2 *>(out + c) = acc[2 * v];
      if (c + 2 < a.n_pad) *reinterpret_cast<double2 *>(out + c + 2) = acc[2 * v + 1];
    }
  }
  if (Op::NS > 0) {
    __syncthreads();
    dev::block_sum<NS, TPB>(sacc, s_red);
    if (t == 0) {
#pragma unroll
      for (int k = 0; k < NS; ++k) a.scalar_partials[static_cast<size_t>(bid) * NS + k] = sacc[k];
    }
  }
}

}  // namespace pogs_amd

// What the Ewald step (ewald_step.hip) and its batched form (ewald_batch.hip) share: the block shapes, the slice rule of the atom
// kernel, the layout of the float64 work area of ONE system, the fixed-order strided sum and the float64 cell inversion (cell_invert.h),
// and on the host the checks of the potential, its constants and the choice of the rows kernel.  The batch lays the work areas
// of its frames one behind the other, each exactly as the single step lays out its own.  The bodies of the seven kernels are
// in ewald_step_bodies.h.
#pragma once

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "cell_invert.h"  // es_invert_cell: the float64 cell inversion
#include "host.h"
#include "kpot.h"
#include "rows_body.h"

namespace mipme {

constexpr int kEsBlock = 256;
constexpr int kEsWaves = kEsBlock / 64;
constexpr int kEsRowsPerBlock = kEsBlock / 16;  // 16 lanes per atom row
static_assert(kRowLanes == 16, "row_sum of rows_body.h adds up the 16 lanes of a row");
static_assert(kCompactAtomBits == kStepRowsAtomBits, "check_step_rows of host.h admits what the 4-byte entries hold");
constexpr int kEsKPerBlock = 8;                 // k-vectors per block of the structure and cell kernels, 32 lanes each
constexpr int kEsKLanes = kEsBlock / kEsKPerBlock;
constexpr int kEsTile = 256;                    // atoms staged per LDS tile of the structure and cell kernels
constexpr int kEsCellK = 10;                    // per k block: W (9), 1/2 sum G |S|^2
constexpr int kEsGeom = 16;                     // geometry record: A^-1 (9, row-major), 1/|det|, bad (0 / 1), padding
constexpr int64_t kEsTargetBlocks = 2048;       // 256 CUs x 8 workgroups
constexpr int64_t kEsMinSlice = 256;            // k-vectors per slice at least (one per thread)
constexpr int64_t kEsMaxK = int64_t(kEsKPerBlock) * 0x7fffffff;

static int64_t es_slices(int64_t N, int64_t K) {
  if (N <= 0 || K <= 0) return 0;
  int64_t s = (kEsTargetBlocks + N - 1) / N;
  s = std::min<int64_t>(s, std::max<int64_t>(1, K / kEsMinSlice));
  return std::max<int64_t>(1, std::min<int64_t>(s, 65535));
}

// work (float64 slots): [geometry 16][q partials 1 per atom block][energy partials 1 per finish block]
//                       [row cell partials 9 per row block][k cell partials 10 per k block][row results 4 N (values of T)]
//                       [slice partials 4 N S (values of T)]
struct EsWork {
  int64_t n_table_blocks, n_atom_blocks, n_fin_blocks, n_row_blocks, n_k_blocks, n_slices;
  double *geom, *q_part, *e_part, *row_cell, *k_cell;
  void *row_out, *slice_part;
  int64_t total;
};
static EsWork es_work_layout(int64_t N, int64_t K, bool cell, void* base) {
  EsWork w;
  w.n_table_blocks = std::max<int64_t>(1, (K + kEsBlock - 1) / kEsBlock);  // (block 0 writes the geometry: at least one)
  w.n_atom_blocks = (N + kEsBlock - 1) / kEsBlock;
  w.n_fin_blocks = (N + kEsRowsPerBlock - 1) / kEsRowsPerBlock;
  w.n_row_blocks = cell ? w.n_fin_blocks : 0;
  w.n_k_blocks = cell ? (K + kEsKPerBlock - 1) / kEsKPerBlock : 0;
  w.n_slices = es_slices(N, K);
  double* b = (double*)base;
  w.geom = b;
  w.q_part = w.geom + kEsGeom;
  w.e_part = w.q_part + w.n_atom_blocks;
  w.row_cell = w.e_part + w.n_fin_blocks;
  w.k_cell = w.row_cell + 9 * w.n_row_blocks;
  double* row_out = w.k_cell + kEsCellK * w.n_k_blocks;
  double* slice_part = row_out + 4 * N;
  w.row_out = row_out;
  w.slice_part = slice_part;
  w.total = kEsGeom + w.n_atom_blocks + w.n_fin_blocks + 9 * w.n_row_blocks + kEsCellK * w.n_k_blocks + 4 * N + 4 * N * w.n_slices;
  return w;
}

// ---- host: what mipme_ewald_step and mipme_ewald_batch check and prepare alike ------------------------------------------------
// the first refusals of both entry points, in this order
inline int check_ewald_pot(int dtype, const mipme_potential_t* pot, const char* who) {
  MIPME_REQUIRE(dtype == MIPME_F32 || dtype == MIPME_F64, "%s: invalid dtype %d", who, int(dtype));
  MIPME_REQUIRE(pot != nullptr, "%s: potential descriptor is NULL", who);
  MIPME_REQUIRE(pot->smearing > 0,
                "%s: the potential has no smearing (`smearing` is %g): the Ewald sum needs a range-separated potential", who,
                pot->smearing);
  MIPME_REQUIRE(!(pot->exclusion_radius > 0) || pot->exclusion_degree >= 1, "%s: exclusion_degree must be >= 1, got %d", who,
                int(pot->exclusion_degree));
  return MIPME_OK;
}

// the constants of the potential in the launches: the fast pair function, the self term and the background term
struct EsTerms {
  FastRS cf;
  double self_c, bg;
};
inline EsTerms es_terms(const mipme_potential_t* pot, const KPot& kp, const SRPot& sp) {
  EsTerms t;
  t.cf = make_fast_rs(sp);
  double bg_c;
  correction_terms(pot, t.self_c, bg_c);
  t.bg = bg_c - 0.5 * kp.k0;  // (the k = 0 term of the eager sum: v_LR(0) Q / V per atom, non-zero for p > 3)
  return t;
}

// launch(PFAST, CELL) with the template arguments of the rows kernel as integral constants
template <typename Launch>
void es_rows_dispatch(const SRPot& sp, bool cell, Launch&& launch) {
  auto with_cell = [&](auto pfast) {
    if (cell)
      launch(pfast, std::true_type{});
    else
      launch(pfast, std::false_type{});
  };
  switch (fast_rs_exponent(sp)) {
    case 1: with_cell(std::integral_constant<int, 1>{}); break;
    case 6: with_cell(std::integral_constant<int, 6>{}); break;
    default: with_cell(std::integral_constant<int, 0>{}); break;
  }
}

// sum_b p[b * stride + off], b < n: thread t adds b = t, t + 256, ... in that order, then the threads in a fixed order
__device__ __forceinline__ double es_strided_sum(const double* __restrict__ p, int64_t n, int stride, int off, double* red) {
  double s = 0.0;
  for (int64_t b = threadIdx.x; b < n; b += kEsBlock) s += p[b * stride + off];
  return block_sum<kEsWaves>(s, red);
}

}  // namespace mipme

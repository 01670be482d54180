// What the Ewald step (ewald_step.hip) and its batched form (ewald_batch.hip) share beyond the skeleton of step_device.h (block
// shapes, slice rule, work layout, strided sum): the head of the float64 work area of ONE system, the float64 cell inversion
// (cell_invert.h), and on the host the checks of the potential, its constants and the choice of the rows kernel.  The batch lays
// the work areas of its frames one behind the other, each exactly as the single step lays out its own.  The bodies of the seven
// kernels are in ewald_step_bodies.h.
#pragma once

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "cell_invert.h"  // es_invert_cell: the float64 cell inversion
#include "host.h"
#include "kpot.h"
#include "rows_body.h"
#include "step_device.h"

namespace mipme {

constexpr int kEsBlock = kStepBlock, kEsKPerBlock = kStepKPerBlock;  // (the names the kernels and launches of the two sources use)
constexpr int kEsGeom = 16;           // geometry record: A^-1 (9, row-major), 1/|det|, bad (0 / 1), padding
constexpr int64_t kEsMinSlice = 256;  // k-vectors per slice at least (one per thread)
constexpr int64_t kEsMaxK = int64_t(kStepKPerBlock) * 0x7fffffff;

// work: the layout of step_device.h behind the geometry record: [geometry 16][q partials 1 per atom block] ... [row results 4 N]
// [slice partials 4 N S]
struct EsWork : StepWork {
  int64_t n_table_blocks;
  double *geom, *q_part;
};
static EsWork es_work_layout(int64_t N, int64_t K, bool cell, void* base) {
  EsWork w{step_work_layout(N, K, cell, base, kEsGeom, 1, 4, kEsMinSlice)};
  w.n_table_blocks = std::max<int64_t>(1, (K + kStepBlock - 1) / kStepBlock);  // (block 0 writes the geometry: at least one)
  w.geom = w.head, w.q_part = w.atom_part;
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

}  // namespace mipme

// What the graphed steps share around their pair physics -- the dipole step (dipole_step.hip), the Ewald step and its batch
// (ewald_step_bodies.h) and, for the block shapes and the shift-table fill, the combined step (combined_step.hip) -- each piece
// defined ONCE: block shapes, slice rule, work layout, strided sum, row front, shift decode, totals of the final kernels.
// Nothing here chooses a grid, declares LDS or launches.
#pragma once

#include <algorithm>
#include <cstdint>

#include "host.h"
#include "rows_body.h"

namespace mipme {

constexpr int kStepBlock = 256;
constexpr int kStepWaves = kStepBlock / 64;
constexpr int kStepRowsPerBlock = kStepBlock / 16;  // 16 lanes per atom row
static_assert(kRowLanes == 16, "row_sum of rows_body.h adds up the 16 lanes of a row");
static_assert(kCompactAtomBits == kStepRowsAtomBits, "check_step_rows of host.h admits what the 4-byte entries hold");
constexpr int kStepKPerBlock = 8;                   // k-vectors per block of the structure and cell kernels, 32 lanes each
constexpr int kStepKLanes = kStepBlock / kStepKPerBlock;
constexpr int kStepTile = 256;                      // atoms staged per LDS tile of the structure and cell kernels
constexpr int kStepCellK = 10;                      // per k block: W (9), 1/2 sum G |S|^2
constexpr int64_t kStepTargetBlocks = 2048;         // 256 CUs x 8 workgroups

// ---- host: slices of the atom kernel and the float64 work area of ONE system ---------------------------------------------------
// min_slice: k-vectors per slice at least
inline int64_t step_slices(int64_t N, int64_t K, int64_t min_slice) {
  if (N <= 0 || K <= 0) return 0;
  int64_t s = (kStepTargetBlocks + N - 1) / N;
  s = std::min<int64_t>(s, std::max<int64_t>(1, K / min_slice));
  return std::max<int64_t>(1, std::min<int64_t>(s, 65535));
}

// work (float64 slots): [head][atom partials P per atom block][energy partials 1 per finish block]
//                       [row cell partials 9 per row block][k cell partials 10 per k block][row results C N (values of T)]
//                       [slice partials C N S (values of T)]
struct StepWork {
  int64_t n_atom_blocks, n_fin_blocks, n_row_blocks, n_k_blocks, n_slices;
  double *head, *atom_part, *e_part, *row_cell, *k_cell;
  void *row_out, *slice_part;
  int64_t total;
};
inline StepWork step_work_layout(int64_t N, int64_t K, bool cell, void* base, int head, int P, int C, int64_t min_slice) {
  StepWork w;
  w.n_atom_blocks = (N + kStepBlock - 1) / kStepBlock;
  w.n_fin_blocks = (N + kStepRowsPerBlock - 1) / kStepRowsPerBlock;
  w.n_row_blocks = cell ? w.n_fin_blocks : 0;
  w.n_k_blocks = cell ? (K + kStepKPerBlock - 1) / kStepKPerBlock : 0;
  w.n_slices = step_slices(N, K, min_slice);
  w.head = (double*)base;
  w.atom_part = w.head + head;
  w.e_part = w.atom_part + P * w.n_atom_blocks;
  w.row_cell = w.e_part + w.n_fin_blocks;
  w.k_cell = w.row_cell + 9 * w.n_row_blocks;
  double* row_out = w.k_cell + kStepCellK * w.n_k_blocks;
  double* slice_part = row_out + C * N;
  w.row_out = row_out;
  w.slice_part = slice_part;
  w.total = head + P * w.n_atom_blocks + w.n_fin_blocks + 9 * w.n_row_blocks + kStepCellK * w.n_k_blocks + C * N + C * N * w.n_slices;
  return w;
}

// ---- device --------------------------------------------------------------------------------------------------------------------
// sum_b p[b * stride + off], b < n: thread t adds b = t, t + 256, ... in that order, then the threads in a fixed order
__device__ __forceinline__ double step_strided_sum(const double* __restrict__ p, int64_t n, int stride, int off, double* red) {
  double s = 0.0;
  for (int64_t b = threadIdx.x; b < n; b += kStepBlock) s += p[b * stride + off];
  return block_sum<kStepWaves>(s, red);
}

// -- row front: 16 lanes per atom row, 4 rows per wavefront; per entry one word (other | code << 22)
// the 7^3 table of Cartesian shift vectors of the DEVICE cell; the caller synchronises
template <typename T>
__device__ __forceinline__ void step_fill_shift_table(AtomRecord<T>* tab, const T* __restrict__ cell) {
  T A[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) A[k] = cell[k];
  fill_shift_table<T, kStepBlock>(tab, A);
}

// the row of this lane: atom a (clamped to N - 1 where the block has no row left: `valid` false, an empty walk), lane `sub` of
// its 16, entries [beg, end) with role i in [beg, mid)
struct StepRow {
  int64_t a;
  bool valid;
  int sub, beg, mid, end;
  unsigned last_atom;  // N - 1: the clamp of step_entry
};
__device__ __forceinline__ StepRow step_row(int64_t N, int64_t blk, const int* __restrict__ row_ptr) {
  StepRow r;
  r.sub = threadIdx.x % 16;
  r.a = blk * kStepRowsPerBlock + threadIdx.x / 16;
  r.valid = r.a < N;
  if (!r.valid) r.a = N - 1;
  const int* __restrict__ rp = row_ptr + 2 * r.a;
  r.beg = rp[0], r.mid = rp[1], r.end = r.valid ? rp[2] : r.beg;
  r.last_atom = unsigned(N - 1);
  return r;
}

// entry e of the row: partner o and shift code; !ok (e beyond the row's end): a real entry that the caller leaves out of its sums
struct StepEntry {
  bool ok;
  unsigned o, code;
};
__device__ __forceinline__ StepEntry step_entry(const int* __restrict__ ent32, int e, const StepRow& r) {
  StepEntry en;
  en.ok = e < r.end;
  const unsigned word = unsigned(ent32[en.ok ? e : r.beg]);  // (beg < end here)
  // (a valid stream never needs the two clamps; they keep a damaged one inside the system's records and the table)
  en.o = min(word & unsigned(kCompactMaxAtoms - 1), r.last_atom);
  en.code = min(word >> kCompactAtomBits, unsigned(kShiftTableSize - 1));
  return en;
}

// the integer shift (sx, sy, sz) of table code `code`: what the role-i virial of the rows kernels multiplies the pair term with
template <typename T>
__device__ __forceinline__ void step_shift_of_code(unsigned code, T& sx, T& sy, T& sz) {
  const int ic = int(code);
  sx = T(ic % kShiftTableBase - kShiftTableRange), sy = T((ic / kShiftTableBase) % kShiftTableBase - kShiftTableRange);
  sz = T(ic / (kShiftTableBase * kShiftTableBase) - kShiftTableRange);
}

// -- totals of the final kernels (one block): tot[0..8] the row cell partials, tot[9..18] the k cell partials (W, then E_raw);
// the caller adds what is its own behind them and synchronises
__device__ __forceinline__ void step_cell_totals(const double* __restrict__ row_cell, int64_t n_row_blocks,
                                                 const double* __restrict__ k_cell, int64_t n_k_blocks, double* tot, double* red) {
  for (int j = 0; j < 9; ++j) {
    const double s = step_strided_sum(row_cell, n_row_blocks, 9, j, red);
    if (threadIdx.x == 0) tot[j] = s;
  }
  for (int j = 0; j < kStepCellK; ++j) {
    const double s = step_strided_sum(k_cell, n_k_blocks, kStepCellK, j, red);
    if (threadIdx.x == 0) tot[9 + j] = s;
  }
}

}  // namespace mipme

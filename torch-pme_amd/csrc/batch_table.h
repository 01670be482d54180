// The frame table of the batched steps (ewald_batch.hip, dipole_batch.hip), defined ONCE: F frames of different sizes in flat
// launches, a table that maps every workgroup to (frame, local block).  Built on the host from sizes alone:
//   [EbFrame x F][prep blocks][k blocks (structure, cell k)][atom blocks][row blocks (rows, finish)]     (EbBlock = frame, local)
// A frame's record holds where its slices of the concatenated buffers begin and where the parts of its work area lie; the work
// area of a frame is laid out exactly as the single step lays out its own (step_work_layout of step_device.h with the constants
// of the step: EbShape), the areas one behind the other in frame order.  Host code only: nothing here is compiled for the device
// but the two structs the kernels read.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>

#include "rows_body.h"
#include "step_device.h"

namespace mipme {

constexpr int kEbMaxFrames = 1 << 20;
constexpr int64_t kEbMaxBlocks = (int64_t(1) << 24) - 1;  // workgroups per launch: 256 threads each, fewer than 2^32 threads
constexpr int64_t kEbMaxSum = 0x7fffffff;                 // sum of the atoms, of the k-vectors, of the entries: int32 on the host side

// One frame of the table.  Offsets count from the start of the concatenated buffers (atoms, k-vectors, row pointers, entries) and
// of the work area (float64 slots).  atom_part: the float64 partials per atom block (charges: 1, dipoles: 3).
struct EbFrame {
  int64_t atom0, n_atoms, k0, n_k, rp0, ent0, chunk;
  int64_t geom, atom_part, e_part, row_cell, k_cell, row_out, slice_part;
  int32_t n_table_blocks, n_atom_blocks, n_fin_blocks, n_row_blocks, n_k_blocks, n_slices;
  int32_t ns[3], _pad;
};
static_assert(sizeof(EbFrame) == 152, "the table_bytes functions document 152 bytes per frame");
struct EbBlock {
  int32_t frame, local;
};
static_assert(sizeof(EbBlock) == 8, "the table_bytes functions document 8 bytes per workgroup");

struct EbLayout {
  int64_t n_prep, n_kblk, n_atomblk, n_rowblk;  // workgroups of the launches
  int64_t sum_atoms, sum_k, work_total, table_bytes;
};

// The constants of the step whose frames the table lays out: the arguments of step_work_layout.
struct EbShape {
  int head, atom_partials, results;  // float64 slots of the head; partials per atom block; results per atom
  int64_t min_slice;                 // k-vectors per slice of the atom launch at least
};

// The sizes decide everything: false for sizes the batch does not serve.  frames / blocks (nullable): the host table to fill.
static bool eb_layout(const EbShape& shape, int F, const int64_t* atom_ptr, const int64_t* k_ptr, const int64_t* entry_ptr,
                      const int32_t* ns, bool cell, EbLayout& L, EbFrame* frames, EbBlock* blocks) {
  L = EbLayout{};
  if (F < 1 || F > kEbMaxFrames || !atom_ptr || !k_ptr || atom_ptr[0] != 0 || k_ptr[0] != 0) return false;
  if (entry_ptr && entry_ptr[0] != 0) return false;
  const auto layout = [&](int64_t N, int64_t K) {
    return step_work_layout(N, K, cell, nullptr, shape.head, shape.atom_partials, shape.results, shape.min_slice);
  };
  const auto table_blocks = [](int64_t K) {
    return std::max<int64_t>(1, (K + kStepBlock - 1) / kStepBlock);  // (block 0 writes the geometry: at least one)
  };
  for (int f = 0; f < F; ++f) {
    const int64_t N = atom_ptr[f + 1] - atom_ptr[f], K = k_ptr[f + 1] - k_ptr[f];
    if (N < 1 || N > kCompactMaxAtoms || K < 0 || K > kEbMaxSum) return false;
    if (atom_ptr[f + 1] > kEbMaxSum || k_ptr[f + 1] > kEbMaxSum) return false;
    if (entry_ptr && (entry_ptr[f + 1] - entry_ptr[f] < 1 || entry_ptr[f + 1] > kEbMaxSum)) return false;  // (2 P_f + 1 words)
    const StepWork w = layout(N, K);
    const int64_t n_k8 = (K + kStepKPerBlock - 1) / kStepKPerBlock;
    L.n_prep += table_blocks(K) + w.n_atom_blocks;
    L.n_kblk += n_k8;
    L.n_atomblk += N * w.n_slices;
    L.n_rowblk += w.n_fin_blocks;
    if (L.n_prep > kEbMaxBlocks || L.n_kblk > kEbMaxBlocks || L.n_atomblk > kEbMaxBlocks || L.n_rowblk > kEbMaxBlocks) return false;
    L.work_total += w.total;
  }
  L.sum_atoms = atom_ptr[F], L.sum_k = k_ptr[F];
  L.table_bytes = int64_t(sizeof(EbFrame)) * F + int64_t(sizeof(EbBlock)) * (L.n_prep + L.n_kblk + L.n_atomblk + L.n_rowblk);
  if (!frames) return true;
  EbBlock* b_prep = blocks;
  EbBlock* b_k = b_prep + L.n_prep;
  EbBlock* b_atom = b_k + L.n_kblk;
  EbBlock* b_row = b_atom + L.n_atomblk;
  int64_t work0 = 0;
  for (int f = 0; f < F; ++f) {
    const int64_t N = atom_ptr[f + 1] - atom_ptr[f], K = k_ptr[f + 1] - k_ptr[f];
    const StepWork w = layout(N, K);
    const int64_t n_k8 = (K + kStepKPerBlock - 1) / kStepKPerBlock, n_table = table_blocks(K);
    EbFrame& r = frames[f];
    memset(&r, 0, sizeof(r));
    r.atom0 = atom_ptr[f], r.n_atoms = N, r.k0 = k_ptr[f], r.n_k = K;
    r.rp0 = 2 * atom_ptr[f] + f;  // (2 N + 1 row pointers per frame)
    r.ent0 = entry_ptr[f];
    r.chunk = w.n_slices > 0 ? (K + w.n_slices - 1) / w.n_slices : 0;
    r.geom = work0 + (w.head - (double*)nullptr);
    r.atom_part = work0 + (w.atom_part - (double*)nullptr);
    r.e_part = work0 + (w.e_part - (double*)nullptr);
    r.row_cell = work0 + (w.row_cell - (double*)nullptr);
    r.k_cell = work0 + (w.k_cell - (double*)nullptr);
    r.row_out = work0 + ((double*)w.row_out - (double*)nullptr);
    r.slice_part = work0 + ((double*)w.slice_part - (double*)nullptr);
    r.n_table_blocks = int32_t(n_table), r.n_atom_blocks = int32_t(w.n_atom_blocks), r.n_fin_blocks = int32_t(w.n_fin_blocks);
    r.n_row_blocks = int32_t(w.n_row_blocks), r.n_k_blocks = int32_t(w.n_k_blocks), r.n_slices = int32_t(w.n_slices);
    r.ns[0] = ns[3 * f], r.ns[1] = ns[3 * f + 1], r.ns[2] = ns[3 * f + 2];
    for (int64_t b = 0; b < n_table + w.n_atom_blocks; ++b) *b_prep++ = EbBlock{f, int32_t(b)};
    for (int64_t b = 0; b < n_k8; ++b) *b_k++ = EbBlock{f, int32_t(b)};
    for (int64_t b = 0; b < N * w.n_slices; ++b) *b_atom++ = EbBlock{f, int32_t(b)};
    for (int64_t b = 0; b < w.n_fin_blocks; ++b) *b_row++ = EbBlock{f, int32_t(b)};
    work0 += w.total;
  }
  return true;
}

}  // namespace mipme

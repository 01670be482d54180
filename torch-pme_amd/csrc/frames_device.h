// The per-frame record of the frame batches (frames.hip, frames_cell.hip, frames_slab.hip): every kernel of a batch reads its frame's arguments from
// a device-resident table of these, built once per batch (mipme_frames_table_build / mipme_frames_table_contract).
#pragma once
#include "bricks_device.h"

namespace mipme {
template <typename T>
struct FrameDev {
  // binning
  Geom g;
  BrickGeom bg;
  int64_t N;
  const T* pos;
  const T* q;
  BinIndex bins;  // live = the frame's brick counters
  int* over_brick;
  int4* rec;
  T* wts;
  AtomRecord<T>* atom_rec;
  int even;
  // spread + pair sum
  SpreadArgs<T> spread;
  FusedRowsArgs<T> rows;
  unsigned n_row_blocks;
  // gather
  const T* phi_mesh;
  const T* dc;
  T inv_vol, self_c, bg_c;
  T* out;
  T* field;
  // energy, forces
  T* energy;
  const T* force;
  T* grad_pos;
  T force_scale;  // 1/2 for a full list
  // gather tail (energy + forces in the gather launch)
  GatherTail<T> tail;
  bool use_tail;
};

// the frames table: n_frames FrameDev<T>, then n_frames FrameCellRec (filled by mipme_frames_table_contract, zero otherwise)
template <typename T>
inline FrameCellRec* frames_cell_recs(const void* table, int n_frames) {
  static_assert(sizeof(FrameDev<T>) % 8 == 0, "the cell records follow the frame records");
  return (FrameCellRec*)((char*)const_cast<void*>(table) + size_t(n_frames) * sizeof(FrameDev<T>));
}

// frames.hip: what every entry point of the frame batches refuses of its frames before anything else
int frames_check(int dtype, int n_frames, const mipme_frame_t* fr);

// frames_cells.hip: the cells of a batch as a replay input -- the status word of every frame on its gather tail (host table), and
// the ONE launch that turns the cells on the device into the table's geometry fields, the filter tables and the validated copy
template <typename T> int frames_table_cells_t(int n_frames, void* host_table, void* status);
template <typename T> int frames_cells_launch(hipStream_t st, int n_frames, const mipme_mesh_t* m, const mipme_potential_t* pot,
                                              void* device_table, const void* cells_in, void* cells_valid, void* G, int64_t G_stride,
                                              void* G_deriv, int64_t G_deriv_stride, double mesh_spacing, void* status);

// frames_cell.hip: the co-scheduled launches of a batch whose pair sum also forms the cell sums (FusedRowsArgs::cpart of every
// frame; 4-byte entries, 1/r or 1/r^6: rows_cell_supported) -- the plane route and the brick route
template <typename T> int frames_cell_plane_rows(hipStream_t st, int scheme, int order, int pfast, dim3 grid, size_t lds,
                                                 const FrameDev<T>* table, const PlaneArgs<T>& pa, int64_t frame_stride);
template <typename T> int frames_cell_spread_rows(hipStream_t st, int scheme, int order, int pfast, dim3 grid, size_t lds, const FrameDev<T>* table);

// frames_slab.hip: the launches of a batch with the 2-D periodic (slab) term (mipme_frames_table_slab / mipme_frames_slab_step) --
// the moments {Q, sum q z, sum q z^2} of every frame in one launch, grid (blocks <= kSlabBlocks, frames), and the gather + tail
// compiled with the term (gather_brick_body<SLAB>)
template <typename T> int frames_slab_moments(hipStream_t st, const FrameDev<T>* table, int n_frames, int64_t max_atoms);
template <typename T> int frames_slab_gather_tail(hipStream_t st, int scheme, int order, dim3 grid, const FrameDev<T>* table,
                                                  const double* epart_k, int n_k);

}  // namespace mipme

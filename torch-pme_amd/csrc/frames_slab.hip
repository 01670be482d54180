// The launches of a frame batch with the 2-D periodic (slab) term of the reference (potentials/coulomb.py:6-40; GatherTail in
// bricks_device.h has the formulas): mipme_frames_table_slab attaches the per-frame state, mipme_frames_slab_step runs these.
// A translation unit of its own, like frames_cell.hip and for the same reason: the kernels of frames.hip and frames_cell.hip stay
// what they were, and a batch without the term launches none of these.
#include "cell_finalize_device.h"
#include "frames_device.h"

namespace mipme {

// Moments of every frame in one launch: blockIdx.y = frame, each with its own work slice (tail.slab_mom: {Q, M, M2}, the block
// sums, the ticket).  z is the Cartesian coordinate along the frame's own axis.  The launch is the FIRST of the step and reads
// the caller's positions and charges (strides 3, 1) -- not the records, which the binning launch behind it writes -- so that
// nothing of the step waits for it before the gather.  The grid is sized by the largest frame; a block without atoms of its
// frame adds zeros and still draws its ticket.  A fully periodic frame of a mixed batch (c0 = 0) forms no sums: its moments stay
// the zeros its work slice was allocated with.
template <typename T>
__global__ __launch_bounds__(256) void frames_slab_moments_kernel(const FrameDev<T>* __restrict__ table) {
  const FrameDev<T>& f = table[blockIdx.y];
  if (f.tail.slab_c0 == 0.0) return;  // (uniform per workgroup)
  slab_moments_body<T>(f.N, f.pos + f.tail.slab_axis, 3, f.q, 1, const_cast<double*>(f.tail.slab_mom), blockIdx.x, gridDim.x);
}

// frames.hip's frames_gather_tail_kernel with the term: potentials, energy and the field of every frame carry it (the stored
// field too, so that mipme_frames_backward with another seed stays correct); the cell sums take the mesh part alone.
template <int N, typename T, bool SLAB>
__global__ __launch_bounds__(GATHER_THREADS) void frames_gather_tail_kernel(const FrameDev<T>* __restrict__ table,
                                                                           const double* __restrict__ epart_k, int n_k) {
  static_assert(SLAB, "the instantiation without the term lives in frames.hip");
  const FrameDev<T>& f = table[blockIdx.y];
  GatherTail<T> tail = f.tail;
  tail.epart_k = epart_k + int64_t(blockIdx.y) * n_k;  // the x stage writes one block of partial sums per batch entry
  tail.n_k = n_k;
  gather_brick_body<N, true, T, true, GATHER_THREADS, true>(f.g, f.bg, 1, f.bins, f.rec, f.wts, f.phi_mesh, f.q, f.dc, f.inv_vol,
                                                            f.self_c, f.bg_c, true, f.out, nullptr, f.field, blockIdx.x, &tail);
}

// kfilter.hip's frames_cell_finalize_kernel with the term's cell dependence (through V and L = |a_axis|), from the frame's record
template <typename T, bool SLAB>
__global__ __launch_bounds__(1024) void frames_cell_finalize_kernel(const FrameCellRec* __restrict__ recs) {
  static_assert(SLAB, "the instantiation without the term lives in kfilter.hip");
  const FrameCellRec& f = recs[blockIdx.x];
  cell_tail_finalize_body<T, true>(f.mesh, f.bg, f.pair_scale, f.n_riders, f.n_bricks, f.rows, f.rpart, (const T*)f.dc,
                                   (const T*)f.seed, (T*)f.out, SlabCell{f.slab_mom, f.slab_c0, f.slab_L, f.slab_axis});
}

template <typename T>
int frames_slab_moments(hipStream_t st, const FrameDev<T>* table, int n_frames, int64_t max_atoms) {
  static_assert(kSlabBlocks <= 64, "one wave adds the block sums up");
  const unsigned blocks = unsigned(std::min<int64_t>(kSlabBlocks, (max_atoms + 255) / 256));
  frames_slab_moments_kernel<T><<<dim3(blocks, unsigned(n_frames)), 256, 0, st>>>(table);
  MIPME_LAUNCH_CHECK();
  return MIPME_OK;
}

template <typename T>
int frames_slab_gather_tail(hipStream_t st, int scheme, int order, dim3 grid, const FrameDev<T>* table, const double* epart_k,
                            int n_k) {
  MIPME_DISPATCH_STENCIL_B(scheme, order,
                           ((void)S, frames_gather_tail_kernel<N, T, true><<<grid, GATHER_THREADS, 0, st>>>(table, epart_k, n_k)));
  MIPME_LAUNCH_CHECK();
  return MIPME_OK;
}

template <typename T>
int frames_slab_cell_finalize(hipStream_t st, const FrameCellRec* recs, int n_frames) {
  frames_cell_finalize_kernel<T, true><<<unsigned(n_frames), 1024, 0, st>>>(recs);
  MIPME_LAUNCH_CHECK();
  return MIPME_OK;
}

template int frames_slab_moments<float>(hipStream_t, const FrameDev<float>*, int, int64_t);
template int frames_slab_moments<double>(hipStream_t, const FrameDev<double>*, int, int64_t);
template int frames_slab_gather_tail<float>(hipStream_t, int, int, dim3, const FrameDev<float>*, const double*, int);
template int frames_slab_gather_tail<double>(hipStream_t, int, int, dim3, const FrameDev<double>*, const double*, int);
template int frames_slab_cell_finalize<float>(hipStream_t, const FrameCellRec*, int);
template int frames_slab_cell_finalize<double>(hipStream_t, const FrameCellRec*, int);

}  // namespace mipme

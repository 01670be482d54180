// The co-scheduled launches of a frame batch with the cell gradient (mipme_frames_step, cell_gradient != 0): frames.hip's
// frames_spread_rows_kernel / frames_plane_rows_kernel with the CELL variants of the row bodies.  A translation unit of its own:
// the compiler's inlining decisions for the bodies depend on who else calls them in the module, and the kernels of frames.hip
// stay byte for byte what they were this way.
#include "frames_device.h"

namespace mipme {

// The row workgroups also leave the per-wave cell sums in the frame's cwave slice (FusedRowsArgs::cpart, set by
// mipme_frames_table_contract).  The grid is sized by the largest frame; a frame's row blocks beyond its own N do not run, and its
// riders read the (N + 3) / 4 wavefronts that hold a row, all of which have run.
template <int N, typename T, int PFAST, bool COMPACT, bool CELL>
__global__ __launch_bounds__(SPREAD_THREADS, sizeof(T) == 4 ? MIPME_CELL_WAVES : 1) void frames_spread_rows_kernel(const FrameDev<T>* __restrict__ table) {
  static_assert(CELL && COMPACT, "the cell sums need the 4-byte entries");
  const FrameDev<T>& f = table[blockIdx.y];
  const unsigned n_spread = unsigned(f.bg.nb);
  extern __shared__ __attribute__((aligned(16))) char smem_rows[];  // see spread_rows_kernel
  if (blockIdx.x < n_spread)
    spread_brick_body<N, T>(f.spread, blockIdx.x);
  else if (blockIdx.x - n_spread < f.n_row_blocks)
    cosched_row_block<T, PFAST, true, true>(f.rows, blockIdx.x - n_spread, smem_rows);
}

template <int SCHEME, int N, typename T, int PFAST, bool COMPACT, bool CELL>
__global__ __launch_bounds__(SPREAD_THREADS, sizeof(T) == 4 ? MIPME_CELL_WAVES : 1) void frames_plane_rows_kernel(const FrameDev<T>* __restrict__ table,
                                                                                                   PlaneArgs<T> pa, int64_t frame_stride) {
  static_assert(CELL && COMPACT, "the cell sums need the 4-byte entries");
  const FrameDev<T>& f = table[blockIdx.y];
  const unsigned n_items = unsigned(f.g.nx) * unsigned(pa.parts);
  extern __shared__ __attribute__((aligned(16))) char smem_fp[];
  if (blockIdx.x < n_items) {
    pa.hat += int64_t(blockIdx.y) * frame_stride;
    if (pa.hat_more) pa.hat_more += int64_t(blockIdx.y) * frame_stride;
    plane_spread_yz_body<SCHEME, N, T>(f.spread, pa, blockIdx.x, smem_fp);
  } else if (blockIdx.x - n_items < f.n_row_blocks) {
    cosched_row_block<T, PFAST, true, true>(f.rows, blockIdx.x - n_items, smem_fp);
  }
}

template <typename T>
int frames_cell_plane_rows(hipStream_t st, int scheme, int order, int pfast, dim3 grid, size_t lds, const FrameDev<T>* table,
                           const PlaneArgs<T>& pa, int64_t frame_stride) {
  MIPME_REQUIRE(pfast == 1 || pfast == 6, "the cell sums of the pair kernels cover 1/r and 1/r^6");
  if (pfast == 1)
    MIPME_DISPATCH_STENCIL_B(scheme, order, (frames_plane_rows_kernel<S, N, T, 1, true, true><<<grid, SPREAD_THREADS, lds, st>>>(table, pa, frame_stride)));
  else
    MIPME_DISPATCH_STENCIL_B(scheme, order, (frames_plane_rows_kernel<S, N, T, 6, true, true><<<grid, SPREAD_THREADS, lds, st>>>(table, pa, frame_stride)));
  MIPME_LAUNCH_CHECK();
  return MIPME_OK;
}

template <typename T>
int frames_cell_spread_rows(hipStream_t st, int scheme, int order, int pfast, dim3 grid, size_t lds, const FrameDev<T>* table) {
  MIPME_REQUIRE(pfast == 1 || pfast == 6, "the cell sums of the pair kernels cover 1/r and 1/r^6");
  if (pfast == 1)
    MIPME_DISPATCH_STENCIL_B(scheme, order, ((void)S, frames_spread_rows_kernel<N, T, 1, true, true><<<grid, SPREAD_THREADS, lds, st>>>(table)));
  else
    MIPME_DISPATCH_STENCIL_B(scheme, order, ((void)S, frames_spread_rows_kernel<N, T, 6, true, true><<<grid, SPREAD_THREADS, lds, st>>>(table)));
  MIPME_LAUNCH_CHECK();
  return MIPME_OK;
}

template int frames_cell_plane_rows<float>(hipStream_t, int, int, int, dim3, size_t, const FrameDev<float>*, const PlaneArgs<float>&, int64_t);
template int frames_cell_plane_rows<double>(hipStream_t, int, int, int, dim3, size_t, const FrameDev<double>*, const PlaneArgs<double>&, int64_t);
template int frames_cell_spread_rows<float>(hipStream_t, int, int, int, dim3, size_t, const FrameDev<float>*);
template int frames_cell_spread_rows<double>(hipStream_t, int, int, int, dim3, size_t, const FrameDev<double>*);

}  // namespace mipme

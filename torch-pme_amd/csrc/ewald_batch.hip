// The Ewald step of ewald_step.hip for MANY small systems in one call (mipme_ewald_batch, include/mipme.h): F frames, each with
// its own cell, atom count, k grid and pair list, served by the same launches as one system -- prep, structure, atoms, rows,
// cell k (with the cell gradient), finish, final -- each launched ONCE for the whole batch, on one stream, one after the other.
// At the sizes the explicit Ewald sum is chosen for a step is seven launches of a few dozen workgroups each: latency, not work.
// The batch puts the workgroups of all frames into the same seven launches.
//
// Frames differ in size, so a launch is a FLAT grid and a table maps every workgroup to (frame, local block): no workgroup is
// launched to find that it has nothing to do (one 4 096-atom frame beside 500 frames of 20 atoms costs the sum of their blocks,
// not 501 times the largest), and no workgroup straddles two frames: one shift table per row block, one frame's records per LDS
// tile.  The table (mipme_ewald_batch_table_build) is built on the host from sizes alone -- nothing in it depends on any cell's
// values -- and uploaded once per capture:
//   [EbFrame x F][prep blocks][k blocks (structure, cell k)][atom blocks][row blocks (rows, finish)]     (EbBlock = frame, local)
// A frame's record holds where its slices of the concatenated buffers begin and where its work area lies; the work area of a frame
// is laid out exactly as the single step lays out its own (es_work_layout), the areas one behind the other in frame order.
//
// Inside its blocks a frame is computed as the single step computes it, with LOCAL indices (partner atoms, row pointers and
// k-vectors count from the start of the frame): the slice count of the atom kernel is es_slices(N_f, K_f), every cross-block sum
// is float64 block partials of that frame added in index order by a later launch, and nothing a block reads belongs to another
// frame.  So the bits a frame gets depend on its own inputs alone -- not on its index, on F or on its neighbours in the batch.
// No atomics, no workgroup waits for another.  A singular cell gives ITS frame a zero k table, E = NaN, dE/dcell = NaN and
// status bit 1, and no other frame anything.
#include <cmath>

#include "dipole_device.h"
#include "ewald_step_device.h"
#include "host.h"
#include "kpot.h"
#include "rows_body.h"

namespace mipme {

constexpr int kEbMaxFrames = 1 << 20;
constexpr int64_t kEbMaxBlocks = (int64_t(1) << 24) - 1;  // workgroups per launch: 256 threads each, fewer than 2^32 threads
constexpr int64_t kEbMaxSum = 0x7fffffff;                 // sum of the atoms, of the k-vectors, of the entries: int32 on the host side

// One frame of the table.  Offsets count from the start of the concatenated buffers (atoms, k-vectors, row pointers, entries) and
// of the work area (float64 slots).
struct EbFrame {
  int64_t atom0, n_atoms, k0, n_k, rp0, ent0, chunk;
  int64_t geom, q_part, e_part, row_cell, k_cell, row_out, slice_part;
  int32_t n_table_blocks, n_atom_blocks, n_fin_blocks, n_row_blocks, n_k_blocks, n_slices;
  int32_t ns[3], _pad;
};
static_assert(sizeof(EbFrame) == 152, "mipme_ewald_batch_table_bytes documents 152 bytes per frame");
struct EbBlock {
  int32_t frame, local;
};
static_assert(sizeof(EbBlock) == 8, "mipme_ewald_batch_table_bytes documents 8 bytes per workgroup");

struct EbLayout {
  int64_t n_prep, n_kblk, n_atomblk, n_rowblk;  // workgroups of the launches
  int64_t sum_atoms, sum_k, work_total, table_bytes;
};

// The sizes decide everything: false for sizes the batch does not serve.  frames / blocks (nullable): the host table to fill.
static bool eb_layout(int F, const int64_t* atom_ptr, const int64_t* k_ptr, const int64_t* entry_ptr, const int32_t* ns, bool cell,
                      EbLayout& L, EbFrame* frames, EbBlock* blocks) {
  L = EbLayout{};
  if (F < 1 || F > kEbMaxFrames || !atom_ptr || !k_ptr || atom_ptr[0] != 0 || k_ptr[0] != 0) return false;
  if (entry_ptr && entry_ptr[0] != 0) return false;
  for (int f = 0; f < F; ++f) {
    const int64_t N = atom_ptr[f + 1] - atom_ptr[f], K = k_ptr[f + 1] - k_ptr[f];
    if (N < 1 || N > kCompactMaxAtoms || K < 0 || K > kEbMaxSum) return false;
    if (atom_ptr[f + 1] > kEbMaxSum || k_ptr[f + 1] > kEbMaxSum) return false;
    if (entry_ptr && (entry_ptr[f + 1] - entry_ptr[f] < 1 || entry_ptr[f + 1] > kEbMaxSum)) return false;  // (2 P_f + 1 words)
    const EsWork w = es_work_layout(N, K, cell, nullptr);
    const int64_t n_k8 = (K + kEsKPerBlock - 1) / kEsKPerBlock;
    L.n_prep += w.n_table_blocks + w.n_atom_blocks;
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
    const EsWork w = es_work_layout(N, K, cell, nullptr);
    const int64_t n_k8 = (K + kEsKPerBlock - 1) / kEsKPerBlock;
    EbFrame& r = frames[f];
    memset(&r, 0, sizeof(r));
    r.atom0 = atom_ptr[f], r.n_atoms = N, r.k0 = k_ptr[f], r.n_k = K;
    r.rp0 = 2 * atom_ptr[f] + f;  // (2 N + 1 row pointers per frame)
    r.ent0 = entry_ptr[f];
    r.chunk = w.n_slices > 0 ? (K + w.n_slices - 1) / w.n_slices : 0;
    r.geom = work0 + (w.geom - (double*)nullptr);
    r.q_part = work0 + (w.q_part - (double*)nullptr);
    r.e_part = work0 + (w.e_part - (double*)nullptr);
    r.row_cell = work0 + (w.row_cell - (double*)nullptr);
    r.k_cell = work0 + (w.k_cell - (double*)nullptr);
    r.row_out = work0 + ((double*)w.row_out - (double*)nullptr);
    r.slice_part = work0 + ((double*)w.slice_part - (double*)nullptr);
    r.n_table_blocks = int32_t(w.n_table_blocks), r.n_atom_blocks = int32_t(w.n_atom_blocks), r.n_fin_blocks = int32_t(w.n_fin_blocks);
    r.n_row_blocks = int32_t(w.n_row_blocks), r.n_k_blocks = int32_t(w.n_k_blocks), r.n_slices = int32_t(w.n_slices);
    r.ns[0] = ns[3 * f], r.ns[1] = ns[3 * f + 1], r.ns[2] = ns[3 * f + 2];
    for (int64_t b = 0; b < w.n_table_blocks + w.n_atom_blocks; ++b) *b_prep++ = EbBlock{f, int32_t(b)};
    for (int64_t b = 0; b < n_k8; ++b) *b_k++ = EbBlock{f, int32_t(b)};
    for (int64_t b = 0; b < N * w.n_slices; ++b) *b_atom++ = EbBlock{f, int32_t(b)};
    for (int64_t b = 0; b < w.n_fin_blocks; ++b) *b_row++ = EbBlock{f, int32_t(b)};
    work0 += w.total;
  }
  return true;
}

// ---- 1. prep: per frame the k table and geometry (local blocks < n_table_blocks), records and charge partials (behind them) --
template <typename T>
__global__ __launch_bounds__(kEsBlock) void ewald_batch_prep_kernel(KPot kp, const EbFrame* __restrict__ frames,
                                                                   const EbBlock* __restrict__ blocks, const T* __restrict__ cells,
                                                                   const int* __restrict__ freq_all, const int* __restrict__ mult_all,
                                                                   double lr_wavelength, const T* __restrict__ pos_all,
                                                                   const T* __restrict__ q_all, T* __restrict__ kvec_all,
                                                                   T* __restrict__ G_all, T* __restrict__ dG_all,
                                                                   AtomRecord<T>* __restrict__ rec_all, double* __restrict__ work,
                                                                   int* __restrict__ status) {
  __shared__ double red[kEsWaves];
  const EbBlock blk = blocks[blockIdx.x];  // (uniform per block, like everything read from the frame's record)
  const EbFrame& fr = frames[blk.frame];
  const int64_t N = fr.n_atoms, K = fr.n_k;
  const int n_table_blocks = fr.n_table_blocks;
  if (blk.local >= n_table_blocks) {
    const int64_t a = int64_t(blk.local - n_table_blocks) * kEsBlock + threadIdx.x;
    double qa = 0.0;
    if (a < N) {
      const int64_t ga = fr.atom0 + a;
      const T qv = q_all[ga];
      rec_all[ga] = AtomRecord<T>{pos_all[3 * ga], pos_all[3 * ga + 1], pos_all[3 * ga + 2], qv};
      qa = double(qv);
    }
    const double s = block_sum<kEsWaves>(qa, red);
    if (threadIdx.x == 0) work[fr.q_part + (blk.local - n_table_blocks)] = s;
    return;
  }
  double A[9];
  const EsCell g = es_invert_cell(cells + 9 * int64_t(blk.frame), A);
  if (blk.local == 0 && threadIdx.x == 0) {
    double* __restrict__ geom = work + fr.geom;
    // A^-1 = (A^-T)^T, row-major
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) geom[3 * r + c] = g.recip[3 * c + r];
    geom[9] = g.inv_vol;
    geom[10] = g.bad ? 1.0 : 0.0;
    // bit 0: the eager call would choose another k grid for this cell, ns_d = ceil(|a_d| / lr_wavelength)
    const int ns[3] = {fr.ns[0], fr.ns[1], fr.ns[2]};
    int st = g.bad ? 2 : 0;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const double norm = sqrt(A[3 * d] * A[3 * d] + A[3 * d + 1] * A[3 * d + 1] + A[3 * d + 2] * A[3 * d + 2]);
      if (!(ceil(norm / lr_wavelength) == double(ns[d]))) st |= 1;
    }
    status[blk.frame] = st;
  }
  const int64_t k = int64_t(blk.local) * kEsBlock + threadIdx.x;
  if (k >= K) return;
  const int* __restrict__ freq = freq_all + 3 * fr.k0;
  double kv[3] = {0.0, 0.0, 0.0}, v = 0.0, dv = 0.0;
  if (!g.bad) {  // (a singular cell: a table of zeros, and the final launch writes NaN as the energy)
    const double f0 = double(freq[3 * k]), f1 = double(freq[3 * k + 1]), f2 = double(freq[3 * k + 2]);
#pragma unroll
    for (int n = 0; n < 3; ++n) kv[n] = (2.0 * kPi) * (f0 * g.recip[n] + f1 * g.recip[3 + n] + f2 * g.recip[6 + n]);
    lr_kernel_dev(kp, kv[0] * kv[0] + kv[1] * kv[1] + kv[2] * kv[2], v, dv);
    const double m = double(mult_all[fr.k0 + k]);
    v *= m;
    dv *= m;
  }
  T* __restrict__ kvec = kvec_all + 3 * fr.k0;
  kvec[3 * k] = T(kv[0]), kvec[3 * k + 1] = T(kv[1]), kvec[3 * k + 2] = T(kv[2]);
  G_all[fr.k0 + k] = T(v);
  if (dG_all) dG_all[fr.k0 + k] = T(dv);
}

// ---- 2. structure factors: 32 lanes per k-vector, the frame's records streamed through LDS ------------------------------------
// (the phase function of the atom and cell kernels: see ewald_step_structure_kernel)
template <typename T>
__global__ __launch_bounds__(kEsBlock) void ewald_batch_structure_kernel(const EbFrame* __restrict__ frames,
                                                                        const EbBlock* __restrict__ blocks,
                                                                        const AtomRecord<T>* __restrict__ rec_all,
                                                                        const T* __restrict__ kvec_all, T* __restrict__ Sc_all,
                                                                        T* __restrict__ Ss_all) {
  __shared__ AtomRecord<T> sr[kEsTile];
  const EbBlock blk = blocks[blockIdx.x];
  const EbFrame& fr = frames[blk.frame];
  const int64_t N = fr.n_atoms, K = fr.n_k;
  const AtomRecord<T>* __restrict__ rec = rec_all + fr.atom0;
  const T* __restrict__ kvec = kvec_all + 3 * fr.k0;
  const int al = threadIdx.x % kEsKLanes;
  const int64_t k = int64_t(blk.local) * kEsKPerBlock + threadIdx.x / kEsKLanes;
  const bool valid = k < K;
  const int64_t kc = valid ? k : 0;
  const T kx = kvec[3 * kc], ky = kvec[3 * kc + 1], kz = kvec[3 * kc + 2];
  T ac = T(0), as = T(0);
  for (int64_t base = 0; base < N; base += kEsTile) {
    const int n = int(min<int64_t>(kEsTile, N - base));
    __syncthreads();
    for (int t = threadIdx.x; t < n; t += kEsBlock) sr[t] = rec[base + t];
    __syncthreads();
    for (int i = al; i < n; i += kEsKLanes) {
      const AtomRecord<T> r = sr[i];
      T s, c;
      dipole_phase3(kx, ky, kz, r.x, r.y, r.z, s, c);
      ac += r.w * c;
      as += r.w * s;
    }
  }
#pragma unroll
  for (int off = kEsKLanes / 2; off > 0; off >>= 1) {
    ac += __shfl_xor(ac, off, kEsKLanes);
    as += __shfl_xor(as, off, kEsKLanes);
  }
  if (valid && al == 0) Sc_all[fr.k0 + k] = ac, Ss_all[fr.k0 + k] = as;
}

// ---- 3. fused atom kernel: local block = slice * N + i, atom i against the k-vectors [slice * chunk, (slice + 1) * chunk) ----
// part[(slice N + i) 4 + c] of the frame: c = 0 the potential sum_k G (c S_c + s S_s), c >= 1 the bracket sum_k G k (c S_s - s S_c)
template <typename T>
__global__ __launch_bounds__(kEsBlock) void ewald_batch_atom_kernel(const EbFrame* __restrict__ frames, const EbBlock* __restrict__ blocks,
                                                                   const AtomRecord<T>* __restrict__ rec_all,
                                                                   const T* __restrict__ kvec_all, const T* __restrict__ G_all,
                                                                   const T* __restrict__ Sc_all, const T* __restrict__ Ss_all,
                                                                   double* __restrict__ work) {
  __shared__ T red[kEsWaves][4];
  const EbBlock blk = blocks[blockIdx.x];
  const EbFrame& fr = frames[blk.frame];
  const int64_t N = fr.n_atoms, K = fr.n_k, chunk = fr.chunk;
  const int64_t i = blk.local % N, slice = blk.local / N;
  const T* __restrict__ kvec = kvec_all + 3 * fr.k0;
  const T* __restrict__ G = G_all + fr.k0;
  const T* __restrict__ Sc = Sc_all + fr.k0;
  const T* __restrict__ Ss = Ss_all + fr.k0;
  T* __restrict__ part = (T*)(work + fr.slice_part);
  const int64_t k0 = slice * chunk, k1 = min<int64_t>(K, k0 + chunk);
  const AtomRecord<T> p = rec_all[fr.atom0 + i];
  T phi = T(0), bx = T(0), by = T(0), bz = T(0);
  for (int64_t k = k0 + threadIdx.x; k < k1; k += kEsBlock) {
    const T gk = G[k];
    if (gk == T(0)) continue;  // exact: the term is G(k) times a finite sum
    const T kx = kvec[3 * k], ky = kvec[3 * k + 1], kz = kvec[3 * k + 2];
    const T sc = Sc[k], ss = Ss[k];
    T s, c;
    dipole_phase3(kx, ky, kz, p.x, p.y, p.z, s, c);
    phi += gk * (c * sc + s * ss);
    const T b = gk * (c * ss - s * sc);
    bx += b * kx;
    by += b * ky;
    bz += b * kz;
  }
  phi = wave_sum(phi), bx = wave_sum(bx), by = wave_sum(by), bz = wave_sum(bz);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) red[wave][0] = phi, red[wave][1] = bx, red[wave][2] = by, red[wave][3] = bz;
  __syncthreads();
  if (threadIdx.x < 4) {
    T s = T(0);
#pragma unroll
    for (int w = 0; w < kEsWaves; ++w) s += red[w][threadIdx.x];
    part[(slice * N + i) * 4 + threadIdx.x] = s;
  }
}

// ---- 4. pair rows: 16 lanes per atom row, the 7^3 shift table of the block's frame in LDS ------------------------------------
// (ewald_step_rows_kernel with the frame's slices: the partners and the row pointers are local to the frame)
template <typename T, int PFAST, bool CELL>
__global__ __launch_bounds__(kEsBlock) void ewald_batch_rows_kernel(SRPot sp, FastRS cf, const EbFrame* __restrict__ frames,
                                                                   const EbBlock* __restrict__ blocks,
                                                                   const int* __restrict__ row_ptr_all,
                                                                   const int* __restrict__ ent32_all,
                                                                   const AtomRecord<T>* __restrict__ rec_all,
                                                                   const T* __restrict__ cells, T scale, double* __restrict__ work) {
  __shared__ AtomRecord<T> shift_tab[kShiftTableSize];
  __shared__ double red[kEsWaves][9];
  const int tid = threadIdx.x;
  const EbBlock blk = blocks[blockIdx.x];
  const EbFrame& fr = frames[blk.frame];
  const int64_t N = fr.n_atoms;
  const int* __restrict__ row_ptr = row_ptr_all + fr.rp0;
  const int* __restrict__ ent32 = ent32_all + fr.ent0;
  const AtomRecord<T>* __restrict__ rec = rec_all + fr.atom0;
  T* __restrict__ row_out = (T*)(work + fr.row_out);
  {
    const T* __restrict__ cell = cells + 9 * int64_t(blk.frame);
    T A[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) A[k] = cell[k];
    fill_shift_table<T, kEsBlock>(shift_tab, A);
  }
  __syncthreads();
  const T c_inv2s2 = T(cf.inv_2s2), c1 = T(cf.c1), cpref = T(cf.pref);
  const int sub = tid % 16;
  int64_t a = int64_t(blk.local) * kEsRowsPerBlock + tid / 16;
  const bool valid = a < N;
  if (!valid) a = N - 1;
  const int* __restrict__ rp = row_ptr + 2 * a;
  const int beg = rp[0], mid = rp[1], end = valid ? rp[2] : beg;
  const AtomRecord<T> pa = rec[a];
  const unsigned last_atom = unsigned(N - 1);
  T pot = T(0), fx = T(0), fy = T(0), fz = T(0);
  T w00 = T(0), w01 = T(0), w02 = T(0), w10 = T(0), w11 = T(0), w12 = T(0), w20 = T(0), w21 = T(0), w22 = T(0);
  for (int base = beg; base < end; base += 16) {
    const int e = base + sub;
    const bool ok = e < end;
    const unsigned word = unsigned(ent32[ok ? e : beg]);  // (beg < end here: a real entry, left out of the sums)
    // (a valid stream never needs the two clamps; they keep a damaged one inside the frame's records and the table)
    const unsigned o = min(word & unsigned(kCompactMaxAtoms - 1), last_atom);
    const unsigned code = min(word >> kCompactAtomBits, unsigned(kShiftTableSize - 1));
    const AtomRecord<T> po = rec[o];
    const AtomRecord<T> sh = shift_tab[code];
    const T vx = (po.x - pa.x) + sh.x, vy = (po.y - pa.y) + sh.y, vz = (po.z - pa.z) + sh.z;
    const T d2 = vx * vx + vy * vy + vz * vz;
    T v, dvd;  // v_SR(d) and v_SR'(d) / d
    if constexpr (PFAST > 0) {
      fast_rs_eval<PFAST, true, T>(c_inv2s2, c1, cpref, d2, v, dvd, cf.cheb);
    } else {
      const T d = fsqrt(d2);
      T dv;
      sr_eval<T, true>(sp, d, v, dv);
      dvd = dv / d;
    }
    if (ok) {
      pot += po.w * v;
      const T w = po.w * dvd;
      const T ex = w * vx, ey = w * vy, ez = w * vz;
      fx += ex;
      fy += ey;
      fz += ez;
      if (CELL && e < mid) {  // role i: the listed pair, its own shift
        const int ic = int(code);
        const T sx = T(ic % kShiftTableBase - kShiftTableRange), sy = T((ic / kShiftTableBase) % kShiftTableBase - kShiftTableRange),
                sz = T(ic / (kShiftTableBase * kShiftTableBase) - kShiftTableRange);
        w00 += sx * ex, w01 += sx * ey, w02 += sx * ez;
        w10 += sy * ex, w11 += sy * ey, w12 += sy * ez;
        w20 += sz * ex, w21 += sz * ey, w22 += sz * ez;
      }
    }
  }
  pot = row_sum(pot), fx = row_sum(fx), fy = row_sum(fy), fz = row_sum(fz);
  if (sub == 0 && valid) {
    T* o = row_out + 4 * a;
    const T sq = scale * pa.w;
    o[0] = scale * pot, o[1] = sq * fx, o[2] = sq * fy, o[3] = sq * fz;
  }
  if (CELL) {
    const int lane = tid & 63, wave = tid >> 6;
    const double qa = double(pa.w);  // (the rows of a wavefront belong to different atoms: q_a goes in before the wave sum)
    const double s0 = wave_sum(qa * double(w00)), s1 = wave_sum(qa * double(w01)), s2 = wave_sum(qa * double(w02));
    const double s3 = wave_sum(qa * double(w10)), s4 = wave_sum(qa * double(w11)), s5 = wave_sum(qa * double(w12));
    const double s6 = wave_sum(qa * double(w20)), s7 = wave_sum(qa * double(w21)), s8 = wave_sum(qa * double(w22));
    if (lane == 0) {
      red[wave][0] = s0, red[wave][1] = s1, red[wave][2] = s2;
      red[wave][3] = s3, red[wave][4] = s4, red[wave][5] = s5;
      red[wave][6] = s6, red[wave][7] = s7, red[wave][8] = s8;
    }
    __syncthreads();
    if (tid < 9) {
      double s = 0.0;
#pragma unroll
      for (int w = 0; w < kEsWaves; ++w) s += red[w][tid];
      work[fr.row_cell + 9 * int64_t(blk.local) + tid] = double(scale) * s;
    }
  }
}

// ---- 5. per-k cell gradient: 32 lanes per k-vector, the frame's records streamed through LDS -------------------------------
// (ewald_step_cellk_kernel: k_part[10 b + 3 a + n] = sum over the k-vectors of local block b of gk_a k_n, [10 b + 9] = sum 1/2 G |S|^2)
template <typename T>
__global__ __launch_bounds__(kEsBlock) void ewald_batch_cellk_kernel(const EbFrame* __restrict__ frames, const EbBlock* __restrict__ blocks,
                                                                    const AtomRecord<T>* __restrict__ rec_all,
                                                                    const T* __restrict__ kvec_all, const T* __restrict__ G_all,
                                                                    const T* __restrict__ dG_all, const T* __restrict__ Sc_all,
                                                                    const T* __restrict__ Ss_all, double* __restrict__ work) {
  __shared__ AtomRecord<T> sr[kEsTile];
  __shared__ double red[kEsKPerBlock][kEsCellK];
  const EbBlock blk = blocks[blockIdx.x];
  const EbFrame& fr = frames[blk.frame];
  const int64_t N = fr.n_atoms, K = fr.n_k;
  const AtomRecord<T>* __restrict__ rec = rec_all + fr.atom0;
  const T* __restrict__ kvec = kvec_all + 3 * fr.k0;
  const T* __restrict__ G = G_all + fr.k0;
  const T* __restrict__ dG = dG_all + fr.k0;
  const T* __restrict__ Sc = Sc_all + fr.k0;
  const T* __restrict__ Ss = Ss_all + fr.k0;
  const int al = threadIdx.x % kEsKLanes, kl = threadIdx.x / kEsKLanes;
  const int64_t k = int64_t(blk.local) * kEsKPerBlock + kl;
  const bool live = k < K && (G[k] != T(0) || dG[k] != T(0));
  const int64_t kc = k < K ? k : 0;
  const T kx = kvec[3 * kc], ky = kvec[3 * kc + 1], kz = kvec[3 * kc + 2];
  const T lSc = Sc[kc], lSs = Ss[kc];
  T ax = T(0), ay = T(0), az = T(0);
  for (int64_t base = 0; base < N; base += kEsTile) {
    const int n = int(min<int64_t>(kEsTile, N - base));
    __syncthreads();
    for (int t = threadIdx.x; t < n; t += kEsBlock) sr[t] = rec[base + t];
    __syncthreads();
    if (live)
      for (int i = al; i < n; i += kEsKLanes) {
        const AtomRecord<T> r = sr[i];
        T s, c;
        dipole_phase3(kx, ky, kz, r.x, r.y, r.z, s, c);
        const T b = r.w * (c * lSs - s * lSc);
        ax += b * r.x;
        ay += b * r.y;
        az += b * r.z;
      }
  }
#pragma unroll
  for (int off = kEsKLanes / 2; off > 0; off >>= 1) {
    ax += __shfl_xor(ax, off, kEsKLanes);
    ay += __shfl_xor(ay, off, kEsKLanes);
    az += __shfl_xor(az, off, kEsKLanes);
  }
  if (al == 0) {
    double g[3] = {0.0, 0.0, 0.0}, e = 0.0;
    const double kd[3] = {double(kx), double(ky), double(kz)};
    if (live) {
      const double gk = double(G[kc]), s2 = double(lSc) * double(lSc) + double(lSs) * double(lSs), d = double(dG[kc]) * s2;
      g[0] = gk * double(ax) + d * kd[0];
      g[1] = gk * double(ay) + d * kd[1];
      g[2] = gk * double(az) + d * kd[2];
      e = 0.5 * gk * s2;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int n = 0; n < 3; ++n) red[kl][3 * a + n] = g[a] * kd[n];
    red[kl][9] = e;
  }
  __syncthreads();
  if (threadIdx.x < kEsCellK) {
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < kEsKPerBlock; ++q) s += red[q][threadIdx.x];
    work[fr.k_cell + kEsCellK * int64_t(blk.local) + threadIdx.x] = s;
  }
}

// ---- 6. finish: 16 lanes per atom over the frame's slices (ewald_step_finish_kernel) ----------------------------------------
template <typename T>
__global__ __launch_bounds__(kEsBlock) void ewald_batch_finish_kernel(const EbFrame* __restrict__ frames, const EbBlock* __restrict__ blocks,
                                                                     T self_c, double two_bg, const AtomRecord<T>* __restrict__ rec_all,
                                                                     T* __restrict__ forces_all, T* __restrict__ grad_q_all,
                                                                     double* __restrict__ work) {
  __shared__ double red[kEsWaves];
  const EbBlock blk = blocks[blockIdx.x];
  const EbFrame& fr = frames[blk.frame];
  const int64_t N = fr.n_atoms;
  const int n_slices = fr.n_slices;
  const double* __restrict__ geom = work + fr.geom;
  const T* __restrict__ part = (const T*)(work + fr.slice_part);
  const T* __restrict__ row_out = (const T*)(work + fr.row_out);
  const AtomRecord<T>* __restrict__ rec = rec_all + fr.atom0;
  T* __restrict__ forces = forces_all + 3 * fr.atom0;
  T* __restrict__ grad_q = grad_q_all + fr.atom0;
  const double inv_vol_d = geom[9];
  double Q = 0.0;
  if (two_bg != 0.0) Q = es_strided_sum(work + fr.q_part, fr.n_atom_blocks, 1, 0, red);  // (uniform) the same fixed order in every block
  const T inv_vol = T(inv_vol_d), bg_term = T(two_bg * Q * inv_vol_d);
  const int sub = threadIdx.x % 16;
  const int64_t a = int64_t(blk.local) * kEsRowsPerBlock + threadIdx.x / 16;
  const bool valid = a < N;
  T phi = T(0), b0 = T(0), b1 = T(0), b2 = T(0);
  if (valid)
    for (int s = sub; s < n_slices; s += 16) {
      const T* __restrict__ p = part + (int64_t(s) * N + a) * 4;
      phi += p[0], b0 += p[1], b1 += p[2], b2 += p[3];
    }
  phi = row_sum(phi), b0 = row_sum(b0), b1 = row_sum(b1), b2 = row_sum(b2);
  double e = 0.0;
  if (valid && sub == 0) {
    const T qa = rec[a].w;
    const T* __restrict__ r = row_out + 4 * a;
    const T d = ((inv_vol * phi - self_c * qa) - bg_term) + r[0];
    grad_q[a] = d;
    const T qv = qa * inv_vol;
    forces[3 * a] = r[1] - qv * b0;
    forces[3 * a + 1] = r[2] - qv * b1;
    forces[3 * a + 2] = r[3] - qv * b2;
    e = 0.5 * double(qa) * double(d);
  }
  e = block_sum<kEsWaves>(e, red);
  if (threadIdx.x == 0) work[fr.e_part + blk.local] = e;
}

// ---- 7. final: one block per frame (ewald_step_final_kernel) ----------------------------------------------------------------
template <typename T, bool CELL>
__global__ __launch_bounds__(kEsBlock) void ewald_batch_final_kernel(const EbFrame* __restrict__ frames, double bg,
                                                                    const double* __restrict__ work, T* __restrict__ energies,
                                                                    T* __restrict__ grad_cells) {
  __shared__ double red[kEsWaves];
  __shared__ double tot[9 + kEsCellK + 1];
  const int64_t f = blockIdx.x;
  const EbFrame& fr = frames[f];
  const double* __restrict__ geom = work + fr.geom;
  const bool bad = geom[10] != 0.0;
  const double E = es_strided_sum(work + fr.e_part, fr.n_fin_blocks, 1, 0, red);
  if (threadIdx.x == 0) energies[f] = bad ? T(NAN) : T(E);
  if (CELL) {
    for (int j = 0; j < 9; ++j) {
      const double s = es_strided_sum(work + fr.row_cell, fr.n_row_blocks, 9, j, red);
      if (threadIdx.x == 0) tot[j] = s;
    }
    for (int j = 0; j < kEsCellK; ++j) {
      const double s = es_strided_sum(work + fr.k_cell, fr.n_k_blocks, kEsCellK, j, red);
      if (threadIdx.x == 0) tot[9 + j] = s;
    }
    {
      const double s = es_strided_sum(work + fr.q_part, fr.n_atom_blocks, 1, 0, red);
      if (threadIdx.x == 0) tot[9 + kEsCellK] = s;
    }
    __syncthreads();
    if (threadIdx.x < 9) {
      const int m = threadIdx.x / 3, n = threadIdx.x % 3;
      const double* Wr = tot;
      const double* Wk = tot + 9;
      const double Ek = tot[9 + 9], Q = tot[9 + kEsCellK], inv_vol = geom[9];
      const double e_v = inv_vol * (Ek - bg * Q * Q);  // what scales with 1/V
      double chain = 0.0;
      for (int a = 0; a < 3; ++a) chain += geom[3 * a + m] * Wk[3 * a + n];
      grad_cells[9 * f + 3 * m + n] = bad ? T(NAN) : T(Wr[3 * m + n] - inv_vol * chain - e_v * geom[3 * n + m]);
    }
  }
}

// ---- host --------------------------------------------------------------------------------------------------------------------
template <typename T, int PFAST>
static void ewald_batch_rows_launch(hipStream_t st, const mipme_ewald_batch_args_t& a, const SRPot& sp, const FastRS& cf, unsigned n_blocks,
                                    const EbFrame* frames, const EbBlock* blocks) {
  const T scale = T(a.full_list ? 0.5 : 1.0);
  if (a.cell_gradient)
    ewald_batch_rows_kernel<T, PFAST, true><<<n_blocks, kEsBlock, 0, st>>>(sp, cf, frames, blocks, (const int*)a.row_ptr,
                                                                          (const int*)a.entries, (const AtomRecord<T>*)a.records,
                                                                          (const T*)a.cells, scale, (double*)a.work);
  else
    ewald_batch_rows_kernel<T, PFAST, false><<<n_blocks, kEsBlock, 0, st>>>(sp, cf, frames, blocks, (const int*)a.row_ptr,
                                                                           (const int*)a.entries, (const AtomRecord<T>*)a.records,
                                                                           (const T*)a.cells, scale, (double*)a.work);
}

template <typename T>
static int ewald_batch_t(const mipme_ewald_batch_args_t& a, const EbLayout& L, const KPot& kp, const SRPot& sp) {
  hipStream_t st = (hipStream_t)a.stream;
  const bool cell = a.cell_gradient != 0;
  const EbFrame* frames = (const EbFrame*)a.device_table;
  const EbBlock* b_prep = (const EbBlock*)(frames + a.n_frames);
  const EbBlock* b_k = b_prep + L.n_prep;
  const EbBlock* b_atom = b_k + L.n_kblk;
  const EbBlock* b_row = b_atom + L.n_atomblk;
  AtomRecord<T>* rec = (AtomRecord<T>*)a.records;
  double* work = (double*)a.work;
  const FastRS cf = make_fast_rs(sp);
  double self_c, bg_c;
  correction_terms(a.pot, self_c, bg_c);
  const double bg = bg_c - 0.5 * kp.k0;  // (the k = 0 term of the eager sum: v_LR(0) Q / V per atom, non-zero for p > 3)
  ewald_batch_prep_kernel<T><<<unsigned(L.n_prep), kEsBlock, 0, st>>>(
      kp, frames, b_prep, (const T*)a.cells, (const int*)a.frequencies, (const int*)a.multiplicities, a.lr_wavelength,
      (const T*)a.positions, (const T*)a.charges, (T*)a.kvectors, (T*)a.G, cell ? (T*)a.dG : nullptr, rec, work, (int*)a.status);
  MIPME_LAUNCH_CHECK();
  if (L.n_kblk > 0) {
    ewald_batch_structure_kernel<T><<<unsigned(L.n_kblk), kEsBlock, 0, st>>>(frames, b_k, rec, (const T*)a.kvectors, (T*)a.s_cos,
                                                                            (T*)a.s_sin);
    MIPME_LAUNCH_CHECK();
    ewald_batch_atom_kernel<T><<<unsigned(L.n_atomblk), kEsBlock, 0, st>>>(frames, b_atom, rec, (const T*)a.kvectors, (const T*)a.G,
                                                                          (const T*)a.s_cos, (const T*)a.s_sin, work);
    MIPME_LAUNCH_CHECK();
  }
  switch (fast_rs_exponent(sp)) {
    case 1: ewald_batch_rows_launch<T, 1>(st, a, sp, cf, unsigned(L.n_rowblk), frames, b_row); break;
    case 6: ewald_batch_rows_launch<T, 6>(st, a, sp, cf, unsigned(L.n_rowblk), frames, b_row); break;
    default: ewald_batch_rows_launch<T, 0>(st, a, sp, cf, unsigned(L.n_rowblk), frames, b_row); break;
  }
  MIPME_LAUNCH_CHECK();
  if (cell && L.n_kblk > 0) {
    ewald_batch_cellk_kernel<T><<<unsigned(L.n_kblk), kEsBlock, 0, st>>>(frames, b_k, rec, (const T*)a.kvectors, (const T*)a.G,
                                                                        (const T*)a.dG, (const T*)a.s_cos, (const T*)a.s_sin, work);
    MIPME_LAUNCH_CHECK();
  }
  ewald_batch_finish_kernel<T><<<unsigned(L.n_rowblk), kEsBlock, 0, st>>>(frames, b_row, T(self_c), 2.0 * bg, rec, (T*)a.forces,
                                                                         (T*)a.grad_charges, work);
  MIPME_LAUNCH_CHECK();
  if (cell)
    ewald_batch_final_kernel<T, true><<<unsigned(a.n_frames), kEsBlock, 0, st>>>(frames, bg, work, (T*)a.energies, (T*)a.grad_cells);
  else
    ewald_batch_final_kernel<T, false><<<unsigned(a.n_frames), kEsBlock, 0, st>>>(frames, bg, work, (T*)a.energies, nullptr);
  MIPME_LAUNCH_CHECK();
  return MIPME_OK;
}

}  // namespace mipme

using namespace mipme;

extern "C" {

int64_t mipme_ewald_batch_work(int n_frames, const int64_t* atom_ptr, const int64_t* k_ptr, int cell_gradient) {
  EbLayout L;
  if (!eb_layout(n_frames, atom_ptr, k_ptr, nullptr, nullptr, cell_gradient != 0, L, nullptr, nullptr)) return 0;
  return L.work_total;
}

int64_t mipme_ewald_batch_table_bytes(int n_frames, const int64_t* atom_ptr, const int64_t* k_ptr, int cell_gradient) {
  EbLayout L;
  if (!eb_layout(n_frames, atom_ptr, k_ptr, nullptr, nullptr, cell_gradient != 0, L, nullptr, nullptr)) return 0;
  return L.table_bytes;
}

int mipme_ewald_batch_table_build(int n_frames, const int64_t* atom_ptr, const int64_t* k_ptr, const int64_t* entry_ptr,
                                  const int32_t* ns, int cell_gradient, void* host_table, int64_t host_table_bytes) {
  const char* who = "mipme_ewald_batch_table_build";
  MIPME_REQUIRE(n_frames >= 1 && n_frames <= kEbMaxFrames, "%s: n_frames must be in 1..2^20, got %d", who, n_frames);
  MIPME_REQUIRE(atom_ptr && k_ptr && entry_ptr && ns && host_table, "%s: NULL array", who);
  for (int f = 0; f < n_frames; ++f)
    MIPME_REQUIRE(ns[3 * f] >= 1 && ns[3 * f + 1] >= 1 && ns[3 * f + 2] >= 1, "%s: frame %d: ns must be >= 1, got (%d, %d, %d)", who, f,
                  int(ns[3 * f]), int(ns[3 * f + 1]), int(ns[3 * f + 2]));
  EbLayout L;
  MIPME_REQUIRE(eb_layout(n_frames, atom_ptr, k_ptr, entry_ptr, ns, cell_gradient != 0, L, nullptr, nullptr),
                "%s: sizes the batch does not serve (each frame 1..2^22 atoms, n_k >= 0, at least one entry word; the sums of the atoms, "
                "k-vectors and entries below 2^31; at most 2^24 - 1 workgroups per launch)", who);
  MIPME_REQUIRE(host_table_bytes == L.table_bytes, "%s: host_table_bytes is %lld, mipme_ewald_batch_table_bytes says %lld", who,
                (long long)host_table_bytes, (long long)L.table_bytes);
  EbFrame* frames = (EbFrame*)host_table;
  eb_layout(n_frames, atom_ptr, k_ptr, entry_ptr, ns, cell_gradient != 0, L, frames, (EbBlock*)(frames + n_frames));
  return MIPME_OK;
}

int mipme_ewald_batch(const mipme_ewald_batch_args_t* in) {
  const char* who = "mipme_ewald_batch";
  mipme_ewald_batch_args_t a;
  int rc = load_args(in, a, MIPME_EWALD_BATCH_VERSION, who);
  if (rc) return rc;
  // everything the arguments alone decide, before anything touches a device
  MIPME_REQUIRE(a.dtype == MIPME_F32 || a.dtype == MIPME_F64, "%s: invalid dtype %d", who, int(a.dtype));
  MIPME_REQUIRE(a.pot != nullptr, "%s: potential descriptor is NULL", who);
  MIPME_REQUIRE(a.pot->smearing > 0,
                "%s: the potential has no smearing (`smearing` is %g): the Ewald sum needs a range-separated potential", who,
                a.pot->smearing);
  MIPME_REQUIRE(!(a.pot->exclusion_radius > 0) || a.pot->exclusion_degree >= 1, "%s: exclusion_degree must be >= 1, got %d", who,
                int(a.pot->exclusion_degree));
  MIPME_REQUIRE((a.shift_format & 0xff) == 2 && !(a.shift_format & MIPME_ROWS_PADDED),
                "%s: the rows are read as 4-byte entries, other | code << 22 (shift_format 2), got shift_format %d", who,
                int(a.shift_format));
  MIPME_REQUIRE(a.n_frames >= 1 && a.n_frames <= kEbMaxFrames, "%s: n_frames must be in 1..2^20, got %d", who, int(a.n_frames));
  MIPME_REQUIRE(std::isfinite(a.lr_wavelength) && a.lr_wavelength > 0, "%s: lr_wavelength must be positive, got %g", who, a.lr_wavelength);
  MIPME_REQUIRE(a.atom_ptr && a.k_ptr && a.entry_ptr && a.device_table, "%s: NULL required buffer (atom_ptr, k_ptr, entry_ptr, device_table)",
                who);
  EbLayout L;
  MIPME_REQUIRE(eb_layout(a.n_frames, a.atom_ptr, a.k_ptr, a.entry_ptr, nullptr, a.cell_gradient != 0, L, nullptr, nullptr),
                "%s: sizes the batch does not serve (each frame 1..2^22 atoms, n_k >= 0, at least one entry word; the sums of the atoms, "
                "k-vectors and entries below 2^31; at most 2^24 - 1 workgroups per launch)", who);
  MIPME_REQUIRE(!a.cell_gradient || a.grad_cells, "%s: cell_gradient needs grad_cells", who);
  MIPME_REQUIRE(!a.cell_gradient || L.sum_k == 0 || a.dG, "%s: cell_gradient needs dG (sum of n_k reals of scratch)", who);
  MIPME_REQUIRE(a.positions && a.charges && a.cells && a.row_ptr && a.entries && a.records && a.energies && a.forces && a.grad_charges &&
                    a.status && a.work &&
                    (L.sum_k == 0 || (a.frequencies && a.multiplicities && a.kvectors && a.G && a.s_cos && a.s_sin)),
                "%s: NULL required buffer", who);
  KPot kp;
  SRPot sp;
  if ((rc = make_kpot(a.pot, kp)) || (rc = make_srpot(a.pot, sp))) return rc;
  DT_SWITCH(a.dtype, ewald_batch_t<float>(a, L, kp, sp), ewald_batch_t<double>(a, L, kp, sp));
}

}  // extern "C"

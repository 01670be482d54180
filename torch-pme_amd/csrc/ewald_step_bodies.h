// The seven computations of the Ewald step, each defined ONCE: the body of every kernel of ewald_step.hip (one system, sizes
// and buffers in the kernel arguments, the block index from blockIdx) and of ewald_batch.hip (many frames, sizes, slices and the
// local block index from the frame table).  A body sees one system: its sizes, ITS slices of the buffers and the index of the
// block inside that system's launch; where they come from is the only thing the two kernel families differ in.  What is
// computed is described at the head of ewald_step.hip.  The LDS arrays are declared in the bodies: every body is inlined into
// the one kernel of each family that calls it.
#pragma once

#include <cmath>

#include "dipole_device.h"
#include "ewald_step_device.h"
#include "kpot.h"
#include "rows_body.h"

namespace mipme {

// ---- 1. prep: k table and geometry (blocks blk < n_table_blocks), records and charge partials (the blocks behind them) ----
// status: the ONE word of this system
template <typename T>
__device__ __forceinline__ void es_prep_body(const KPot& kp, int64_t N, int64_t K, int n_table_blocks, int blk,
                                             const T* __restrict__ cell, const int* __restrict__ freq, const int* __restrict__ mult,
                                             int ns0, int ns1, int ns2, double lr_wavelength, const T* __restrict__ pos,
                                             const T* __restrict__ q, T* __restrict__ kvec, T* __restrict__ G, T* __restrict__ dG,
                                             AtomRecord<T>* __restrict__ rec, double* __restrict__ q_part, double* __restrict__ geom,
                                             int* __restrict__ status) {
  __shared__ double red[kStepWaves];
  if (blk >= n_table_blocks) {  // (uniform per block)
    const int64_t a = int64_t(blk - n_table_blocks) * kStepBlock + threadIdx.x;
    double qa = 0.0;
    if (a < N) {
      const T qv = q[a];
      rec[a] = AtomRecord<T>{pos[3 * a], pos[3 * a + 1], pos[3 * a + 2], qv};
      qa = double(qv);
    }
    const double s = block_sum<kStepWaves>(qa, red);
    if (threadIdx.x == 0) q_part[blk - n_table_blocks] = s;
    return;
  }
  double A[9];
  const EsCell g = es_invert_cell(cell, A);
  if (blk == 0 && threadIdx.x == 0) {
    // A^-1 = (A^-T)^T, row-major
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) geom[3 * r + c] = g.recip[3 * c + r];
    geom[9] = g.inv_vol;
    geom[10] = g.bad ? 1.0 : 0.0;
    // bit 0: the eager call would choose another k grid for this cell, ns_d = ceil(|a_d| / lr_wavelength)
    const int ns[3] = {ns0, ns1, ns2};
    int st = g.bad ? 2 : 0;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const double norm = sqrt(A[3 * d] * A[3 * d] + A[3 * d + 1] * A[3 * d + 1] + A[3 * d + 2] * A[3 * d + 2]);
      if (!(ceil(norm / lr_wavelength) == double(ns[d]))) st |= 1;
    }
    status[0] = st;
  }
  const int64_t k = int64_t(blk) * kStepBlock + threadIdx.x;
  if (k >= K) return;
  double kv[3] = {0.0, 0.0, 0.0}, v = 0.0, dv = 0.0;
  if (!g.bad) {  // (a singular cell: a table of zeros, and the final launch writes NaN as the energy)
    const double f0 = double(freq[3 * k]), f1 = double(freq[3 * k + 1]), f2 = double(freq[3 * k + 2]);
#pragma unroll
    for (int n = 0; n < 3; ++n) kv[n] = (2.0 * kPi) * (f0 * g.recip[n] + f1 * g.recip[3 + n] + f2 * g.recip[6 + n]);
    lr_kernel_dev(kp, kv[0] * kv[0] + kv[1] * kv[1] + kv[2] * kv[2], v, dv);
    const double m = double(mult[k]);
    v *= m;
    dv *= m;
  }
  kvec[3 * k] = T(kv[0]), kvec[3 * k + 1] = T(kv[1]), kvec[3 * k + 2] = T(kv[2]);
  G[k] = T(v);
  if (dG) dG[k] = T(dv);
}

// ---- 2. structure factors: 32 lanes per k-vector, the records streamed through LDS -------------------------------------------
// The mapping of ewald_structure_kernel (ewald.hip) for one channel, with the phase of the atom and cell bodies below
// (dipole_phase3: in float the phase is formed and reduced in double).  With a float phase rounded before sincosf, S and the
// (c, s) of the later launches disagree by |k.r| ulps per term: c S_s - s S_c of an atom with its own contribution to S no
// longer cancels, which is the whole force on a single atom.
template <typename T>
__device__ __forceinline__ void es_structure_body(int64_t N, int64_t K, int64_t blk, const AtomRecord<T>* __restrict__ rec,
                                                  const T* __restrict__ kvec, T* __restrict__ Sc, T* __restrict__ Ss) {
  __shared__ AtomRecord<T> sr[kStepTile];
  const int al = threadIdx.x % kStepKLanes;
  const int64_t k = blk * kStepKPerBlock + threadIdx.x / kStepKLanes;
  const bool valid = k < K;
  const int64_t kc = valid ? k : 0;
  const T kx = kvec[3 * kc], ky = kvec[3 * kc + 1], kz = kvec[3 * kc + 2];
  T ac = T(0), as = T(0);
  for (int64_t base = 0; base < N; base += kStepTile) {
    const int n = int(min<int64_t>(kStepTile, N - base));
    __syncthreads();
    for (int t = threadIdx.x; t < n; t += kStepBlock) sr[t] = rec[base + t];
    __syncthreads();
    for (int i = al; i < n; i += kStepKLanes) {
      const AtomRecord<T> r = sr[i];
      T s, c;
      dipole_phase3(kx, ky, kz, r.x, r.y, r.z, s, c);
      ac += r.w * c;
      as += r.w * s;
    }
  }
#pragma unroll
  for (int off = kStepKLanes / 2; off > 0; off >>= 1) {
    ac += __shfl_xor(ac, off, kStepKLanes);
    as += __shfl_xor(as, off, kStepKLanes);
  }
  if (valid && al == 0) Sc[k] = ac, Ss[k] = as;
}

// ---- 3. fused atom body: atom i of N against the k-vectors [slice * chunk, (slice + 1) * chunk) ------------------------------
// part[(slice N + i) 4 + c]: c = 0 the potential sum_k G (c S_c + s S_s), c >= 1 the bracket sum_k G k (c S_s - s S_c)
template <typename T>
__device__ __forceinline__ void es_atom_body(int64_t i, int64_t slice, int64_t N, int64_t K, int64_t chunk,
                                             const AtomRecord<T>* __restrict__ rec, const T* __restrict__ kvec,
                                             const T* __restrict__ G, const T* __restrict__ Sc, const T* __restrict__ Ss,
                                             T* __restrict__ part) {
  __shared__ T red[kStepWaves][4];
  const int64_t k0 = slice * chunk, k1 = min<int64_t>(K, k0 + chunk);
  const AtomRecord<T> p = rec[i];
  T phi = T(0), bx = T(0), by = T(0), bz = T(0);
  for (int64_t k = k0 + threadIdx.x; k < k1; k += kStepBlock) {
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
    for (int w = 0; w < kStepWaves; ++w) s += red[w][threadIdx.x];
    part[(slice * N + i) * 4 + threadIdx.x] = s;
  }
}

// ---- 4. pair rows ----------------------------------------------------------------------------------------------------------
// 16 lanes per atom row, 4 rows per wavefront; the 7^3 table of Cartesian shift vectors in LDS, filled from the device cell; per
// entry one word (other | code << 22) and one 16- or 32-byte record gather (position and charge of the partner).
//   row_out[4 a]         = scale sum_e q_o v_SR(d_e)                               (scale = 1, or 1/2 for a full list; both roles)
//   row_out[4 a + 1 + c] = scale q_a sum_e q_o v_SR'(d_e)/d_e (u_e)_c              (= the pair force on a)
//   cell_part[9 b + 3 m + n] = scale sum over the role-i entries of the rows of block b of S_m q_a q_o v_SR'/d (u_e)_n   (CELL, float64)
// PFAST: the exponent of fast_rs_eval (range separated, no exclusion: 1 or 6), 0: the general sr_eval
template <typename T, int PFAST, bool CELL>
__device__ __forceinline__ void es_rows_body(const SRPot& sp, const FastRS& cf, int64_t N, int64_t blk, const int* __restrict__ row_ptr,
                                             const int* __restrict__ ent32, const AtomRecord<T>* __restrict__ rec,
                                             const T* __restrict__ cell, T scale, T* __restrict__ row_out,
                                             double* __restrict__ cell_part) {
  __shared__ AtomRecord<T> shift_tab[kShiftTableSize];
  __shared__ double red[kStepWaves][9];
  step_fill_shift_table(shift_tab, cell);
  __syncthreads();
  const T c_inv2s2 = T(cf.inv_2s2), c1 = T(cf.c1), cpref = T(cf.pref);
  const StepRow row = step_row(N, blk, row_ptr);
  const AtomRecord<T> pa = rec[row.a];
  T pot = T(0), fx = T(0), fy = T(0), fz = T(0);
  T w00 = T(0), w01 = T(0), w02 = T(0), w10 = T(0), w11 = T(0), w12 = T(0), w20 = T(0), w21 = T(0), w22 = T(0);
  for (int base = row.beg; base < row.end; base += 16) {
    const int e = base + row.sub;
    const StepEntry en = step_entry(ent32, e, row);
    const AtomRecord<T> po = rec[en.o];
    const AtomRecord<T> sh = shift_tab[en.code];
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
    if (en.ok) {
      pot += po.w * v;
      const T w = po.w * dvd;
      const T ex = w * vx, ey = w * vy, ez = w * vz;
      fx += ex;
      fy += ey;
      fz += ez;
      if (CELL && e < row.mid) {  // role i: the listed pair, its own shift
        T sx, sy, sz;
        step_shift_of_code(en.code, sx, sy, sz);
        w00 += sx * ex, w01 += sx * ey, w02 += sx * ez;
        w10 += sy * ex, w11 += sy * ey, w12 += sy * ez;
        w20 += sz * ex, w21 += sz * ey, w22 += sz * ez;
      }
    }
  }
  pot = row_sum(pot), fx = row_sum(fx), fy = row_sum(fy), fz = row_sum(fz);
  if (row.sub == 0 && row.valid) {
    T* o = row_out + 4 * row.a;
    const T sq = scale * pa.w;
    o[0] = scale * pot, o[1] = sq * fx, o[2] = sq * fy, o[3] = sq * fz;
  }
  if (CELL) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
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
      for (int w = 0; w < kStepWaves; ++w) s += red[w][tid];
      cell_part[9 * blk + tid] = double(scale) * s;
    }
  }
}

// ---- 5. per-k cell gradient: 32 lanes per k-vector, the records streamed through LDS ---------------------------------------
// gk = dE_raw/dk = dG |S|^2 k + G sum_j q_j r_j (c S_s - s S_c),  E_raw = 1/2 sum G |S|^2  (E_k = E_raw / V).
//   k_part[10 b + 3 a + n] = sum over the k-vectors of block b of gk_a k_n;   k_part[10 b + 9] = sum 1/2 G |S|^2        (float64)
template <typename T>
__device__ __forceinline__ void es_cellk_body(int64_t N, int64_t K, int64_t blk, const AtomRecord<T>* __restrict__ rec,
                                              const T* __restrict__ kvec, const T* __restrict__ G, const T* __restrict__ dG,
                                              const T* __restrict__ Sc, const T* __restrict__ Ss, double* __restrict__ k_part) {
  __shared__ AtomRecord<T> sr[kStepTile];
  __shared__ double red[kStepKPerBlock][kStepCellK];
  const int al = threadIdx.x % kStepKLanes, kl = threadIdx.x / kStepKLanes;
  const int64_t k = blk * kStepKPerBlock + kl;
  const bool live = k < K && (G[k] != T(0) || dG[k] != T(0));
  const int64_t kc = k < K ? k : 0;
  const T kx = kvec[3 * kc], ky = kvec[3 * kc + 1], kz = kvec[3 * kc + 2];
  const T lSc = Sc[kc], lSs = Ss[kc];
  T ax = T(0), ay = T(0), az = T(0);
  for (int64_t base = 0; base < N; base += kStepTile) {
    const int n = int(min<int64_t>(kStepTile, N - base));
    __syncthreads();
    for (int t = threadIdx.x; t < n; t += kStepBlock) sr[t] = rec[base + t];
    __syncthreads();
    if (live)
      for (int i = al; i < n; i += kStepKLanes) {
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
  for (int off = kStepKLanes / 2; off > 0; off >>= 1) {
    ax += __shfl_xor(ax, off, kStepKLanes);
    ay += __shfl_xor(ay, off, kStepKLanes);
    az += __shfl_xor(az, off, kStepKLanes);
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
  if (threadIdx.x < kStepCellK) {
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < kStepKPerBlock; ++q) s += red[q][threadIdx.x];
    k_part[kStepCellK * blk + threadIdx.x] = s;
  }
}

// ---- 6. finish -----------------------------------------------------------------------------------------------------------
// 16 lanes per atom: lane l adds the slices l, l + 16, ... in that order, then the 16 lanes are added by the shuffle tree of the
// rows (with few atoms there are hundreds of slices: one thread per atom would walk them one dependent load after the other)
template <typename T>
__device__ __forceinline__ void es_finish_body(int64_t N, int n_slices, int64_t blk, T self_c, double two_bg,
                                               const double* __restrict__ geom, const AtomRecord<T>* __restrict__ rec,
                                               const T* __restrict__ part, const T* __restrict__ row_out,
                                               const double* __restrict__ q_part, int64_t n_q_blocks, T* __restrict__ forces,
                                               T* __restrict__ grad_q, double* __restrict__ e_part) {
  __shared__ double red[kStepWaves];
  const double inv_vol_d = geom[9];
  double Q = 0.0;
  if (two_bg != 0.0) Q = step_strided_sum(q_part, n_q_blocks, 1, 0, red);  // (uniform) the same fixed order in every block
  const T inv_vol = T(inv_vol_d), bg_term = T(two_bg * Q * inv_vol_d);
  const int sub = threadIdx.x % 16;
  const int64_t a = blk * kStepRowsPerBlock + threadIdx.x / 16;
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
  e = block_sum<kStepWaves>(e, red);
  if (threadIdx.x == 0) e_part[blk] = e;
}

// ---- 7. final: one block per system ---------------------------------------------------------------------------------------
// energy, grad_cell (CELL) and geom: the system's own
template <typename T, bool CELL>
__device__ __forceinline__ void es_final_body(int64_t n_e_blocks, const double* __restrict__ e_part, T* __restrict__ energy,
                                              int64_t n_row_blocks, const double* __restrict__ row_cell, int64_t n_k_blocks,
                                              const double* __restrict__ k_cell, int64_t n_q_blocks, const double* __restrict__ q_part,
                                              double bg, const double* __restrict__ geom, T* __restrict__ grad_cell) {
  __shared__ double red[kStepWaves];
  __shared__ double tot[9 + kStepCellK + 1];
  const bool bad = geom[10] != 0.0;
  const double E = step_strided_sum(e_part, n_e_blocks, 1, 0, red);
  if (threadIdx.x == 0) energy[0] = bad ? T(NAN) : T(E);
  if (CELL) {
    step_cell_totals(row_cell, n_row_blocks, k_cell, n_k_blocks, tot, red);
    {
      const double s = step_strided_sum(q_part, n_q_blocks, 1, 0, red);
      if (threadIdx.x == 0) tot[9 + kStepCellK] = s;
    }
    __syncthreads();
    if (threadIdx.x < 9) {
      const int m = threadIdx.x / 3, n = threadIdx.x % 3;
      const double* Wr = tot;
      const double* Wk = tot + 9;
      const double Ek = tot[9 + 9], Q = tot[9 + kStepCellK], inv_vol = geom[9];
      const double e_v = inv_vol * (Ek - bg * Q * Q);  // what scales with 1/V
      double chain = 0.0;
      for (int a = 0; a < 3; ++a) chain += geom[3 * a + m] * Wk[3 * a + n];
      grad_cell[3 * m + n] = bad ? T(NAN) : T(Wr[3 * m + n] - inv_vol * chain - e_v * geom[3 * n + m]);
    }
  }
}

}  // namespace mipme

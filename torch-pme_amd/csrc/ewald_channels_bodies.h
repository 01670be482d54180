// The seven computations of the Ewald step for SEVERAL charge channels (2 <= C <= 8 independent systems of charges on the same
// atoms, cell, k grid and pair list), each defined ONCE: the body of every kernel of ewald_channels_step.hip (one system) and of
// ewald_channels_batch.hip (many frames), exactly as ewald_step_bodies.h serves ewald_step.hip and ewald_batch.hip.  What is
// computed is described at the head of ewald_channels_step.hip.
//
// What a channel does NOT change is done once per (atom, k) or per pair entry: the phase (dipole_phase3: in float formed and
// reduced in double) with its sine and cosine, the shift lookup, the distance and the pair function.  A channel adds a few FMAs.
//
// Channels in registers.  Every per-thread array over the channels has the compile-time length CAP, the CAPACITY C is rounded up
// to (2, 4 or 8), and is indexed by fully unrolled loops only: an array indexed by a runtime channel number would live in
// scratch.  The spare channels c >= C of a capacity are never loaded (nothing is read beyond (N, C)), never stored, and left out
// of every sum OVER the channels by a uniform `c < C`: they cost no result bit.  C itself is a kernel argument: it sets the
// strides of the (N, C) arrays, of the channel-major S^c(k) (channel c of k at c K + k) and of the C + 3 results per atom.
// A row of C charges is read one value at a time: C = 3 floats are 12 bytes and a frame's slice starts at atom0 C, so no load
// assumes more than the alignment of one value.
#pragma once

#include <cmath>

#include "dipole_device.h"
#include "ewald_step_bodies.h"
#include "ewald_step_device.h"
#include "kpot.h"
#include "rows_body.h"

namespace mipme {

constexpr int kEcMinChannels = 2, kEcMaxChannels = 8;

// ---- host: the work area of ONE system and the capacity of a channel count -----------------------------------------------------
// work: the layout of es_work_layout with C partials of Q_c per atom block and C + 3 results per atom and per (slice, atom)
static EsWork ec_work_layout(int64_t N, int64_t K, int C, bool cell, void* base) {
  EsWork w{step_work_layout(N, K, cell, base, kEsGeom, C, C + 3, kEsMinSlice)};
  w.n_table_blocks = std::max<int64_t>(1, (K + kStepBlock - 1) / kStepBlock);  // (block 0 writes the geometry: at least one)
  w.geom = w.head, w.q_part = w.atom_part;
  return w;
}

// launch(CAP) with the capacity of C channels as an integral constant
template <typename Launch>
void ec_capacity_dispatch(int C, Launch&& launch) {
  if (C <= 2)
    launch(std::integral_constant<int, 2>{});
  else if (C <= 4)
    launch(std::integral_constant<int, 4>{});
  else
    launch(std::integral_constant<int, 8>{});
}

// ---- device ----------------------------------------------------------------------------------------------------------------------
// the C charges of atom a, zeros in the spare channels
template <typename T, int CAP>
__device__ __forceinline__ void ec_charges(const T* __restrict__ q, int64_t a, int C, T (&out)[CAP]) {
#pragma unroll
  for (int c = 0; c < CAP; ++c) out[c] = c < C ? q[a * C + c] : T(0);
}

// a tile of n atoms from atom `base` on: records into sr, charges transposed into sq[c][i] (the lanes of the loops below read
// consecutive atoms of one channel); the caller synchronises before and after
template <typename T, int CAP>
__device__ __forceinline__ void ec_stage_tile(int C, int64_t base, int n, const AtomRecord<T>* __restrict__ rec,
                                              const T* __restrict__ q, AtomRecord<T>* sr, T (*sq)[kStepTile]) {
  for (int t = threadIdx.x; t < n; t += kStepBlock) sr[t] = rec[base + t];
  for (int t = threadIdx.x; t < n * C; t += kStepBlock) {
    const int i = t / C, c = t - i * C;
    sq[c][i] = q[base * C + t];
  }
}

// ---- 1. prep: k table and geometry (blocks blk < n_table_blocks: es_prep_body), records and charge partials per channel ------
// rec: (x, y, z, 0);  q_part[b C + c]: the sum of q_ac over the atoms of atom block b
template <typename T>
__device__ __forceinline__ void ec_prep_body(const KPot& kp, int C, int64_t N, int64_t K, int n_table_blocks, int blk,
                                             const T* __restrict__ cell, const int* __restrict__ freq, const int* __restrict__ mult,
                                             int ns0, int ns1, int ns2, double lr_wavelength, const T* __restrict__ pos,
                                             const T* __restrict__ q, T* __restrict__ kvec, T* __restrict__ G, T* __restrict__ dG,
                                             AtomRecord<T>* __restrict__ rec, double* __restrict__ q_part, double* __restrict__ geom,
                                             int* __restrict__ status) {
  if (blk < n_table_blocks) {  // (uniform per block) the k-block part of the single-channel body: it touches no atom
    es_prep_body<T>(kp, N, K, n_table_blocks, blk, cell, freq, mult, ns0, ns1, ns2, lr_wavelength, nullptr, nullptr, kvec, G, dG,
                    nullptr, nullptr, geom, status);
    return;
  }
  __shared__ double red[kStepWaves];
  const int64_t b = blk - n_table_blocks, a = b * kStepBlock + threadIdx.x;
  if (a < N) rec[a] = AtomRecord<T>{pos[3 * a], pos[3 * a + 1], pos[3 * a + 2], T(0)};
  for (int c = 0; c < C; ++c) {
    const double s = block_sum<kStepWaves>(a < N ? double(q[a * C + c]) : 0.0, red);
    if (threadIdx.x == 0) q_part[b * C + c] = s;
  }
}

// ---- 2. structure factors: 32 lanes per k-vector, records and charges streamed through LDS, one phase per (k, atom) -----------
// Sc[c K + k] = sum_j q_jc cos(k r_j), Ss likewise.  The phase function is that of the atom and cell bodies below: see the comment
// above es_structure_body.
template <typename T, int CAP>
__device__ __forceinline__ void ec_structure_body(int C, int64_t N, int64_t K, int64_t blk, const AtomRecord<T>* __restrict__ rec,
                                                  const T* __restrict__ q, const T* __restrict__ kvec, T* __restrict__ Sc,
                                                  T* __restrict__ Ss) {
  __shared__ AtomRecord<T> sr[kStepTile];
  __shared__ T sq[CAP][kStepTile];
  const int al = threadIdx.x % kStepKLanes;
  const int64_t k = blk * kStepKPerBlock + threadIdx.x / kStepKLanes;
  const bool valid = k < K;
  const int64_t kc = valid ? k : 0;
  const T kx = kvec[3 * kc], ky = kvec[3 * kc + 1], kz = kvec[3 * kc + 2];
  T ac[CAP], as[CAP];
#pragma unroll
  for (int c = 0; c < CAP; ++c) ac[c] = T(0), as[c] = T(0);
  for (int64_t base = 0; base < N; base += kStepTile) {
    const int n = int(min<int64_t>(kStepTile, N - base));
    __syncthreads();
    ec_stage_tile<T, CAP>(C, base, n, rec, q, sr, sq);
    __syncthreads();
    for (int i = al; i < n; i += kStepKLanes) {
      const AtomRecord<T> r = sr[i];
      T s, co;
      dipole_phase3(kx, ky, kz, r.x, r.y, r.z, s, co);
#pragma unroll
      for (int c = 0; c < CAP; ++c)
        if (c < C) {
          const T qv = sq[c][i];
          ac[c] += qv * co;
          as[c] += qv * s;
        }
    }
  }
#pragma unroll
  for (int c = 0; c < CAP; ++c)
    if (c < C) {
#pragma unroll
      for (int off = kStepKLanes / 2; off > 0; off >>= 1) {
        ac[c] += __shfl_xor(ac[c], off, kStepKLanes);
        as[c] += __shfl_xor(as[c], off, kStepKLanes);
      }
      if (valid && al == 0) Sc[c * K + k] = ac[c], Ss[c * K + k] = as[c];
    }
}

// ---- 3. fused atom body: atom i of N against the k-vectors [slice * chunk, (slice + 1) * chunk) ------------------------------
// part[(slice N + i) (C + 3) + j]: j < C the potential sum_k G (c S_c^j + s S_s^j) of channel j; j = C + n the bracket
// sum_k G k_n (c A_s - s A_c) with A_s = sum_c q_ic S_s^c, A_c likewise: the contraction over the channels is done per k, so
// there are three bracket sums, not 3 C
template <typename T, int CAP>
__device__ __forceinline__ void ec_atom_body(int C, int64_t i, int64_t slice, int64_t N, int64_t K, int64_t chunk,
                                             const AtomRecord<T>* __restrict__ rec, const T* __restrict__ q,
                                             const T* __restrict__ kvec, const T* __restrict__ G, const T* __restrict__ Sc,
                                             const T* __restrict__ Ss, T* __restrict__ part) {
  __shared__ T red[kStepWaves][CAP + 3];
  const int64_t k0 = slice * chunk, k1 = min<int64_t>(K, k0 + chunk);
  const AtomRecord<T> p = rec[i];
  T qa[CAP], phi[CAP];
  ec_charges<T, CAP>(q, i, C, qa);
#pragma unroll
  for (int c = 0; c < CAP; ++c) phi[c] = T(0);
  T bx = T(0), by = T(0), bz = T(0);
  for (int64_t k = k0 + threadIdx.x; k < k1; k += kStepBlock) {
    const T gk = G[k];
    if (gk == T(0)) continue;  // exact: the term is G(k) times a finite sum
    const T kx = kvec[3 * k], ky = kvec[3 * k + 1], kz = kvec[3 * k + 2];
    T s, co;
    dipole_phase3(kx, ky, kz, p.x, p.y, p.z, s, co);
    T a_s = T(0), a_c = T(0);
#pragma unroll
    for (int c = 0; c < CAP; ++c)
      if (c < C) {
        const T sc = Sc[c * K + k], ss = Ss[c * K + k];
        phi[c] += gk * (co * sc + s * ss);
        a_s += qa[c] * ss;
        a_c += qa[c] * sc;
      }
    const T b = gk * (co * a_s - s * a_c);
    bx += b * kx;
    by += b * ky;
    bz += b * kz;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < CAP; ++c) {
    const T v = wave_sum(phi[c]);
    if (lane == 0) red[wave][c] = v;
  }
  bx = wave_sum(bx), by = wave_sum(by), bz = wave_sum(bz);
  if (lane == 0) red[wave][CAP] = bx, red[wave][CAP + 1] = by, red[wave][CAP + 2] = bz;
  __syncthreads();
  if (int(threadIdx.x) < C + 3) {
    const int j = int(threadIdx.x) < C ? int(threadIdx.x) : CAP + (int(threadIdx.x) - C);  // (the brackets lie behind the capacity)
    T s = T(0);
#pragma unroll
    for (int w = 0; w < kStepWaves; ++w) s += red[w][j];
    part[(slice * N + i) * (C + 3) + threadIdx.x] = s;
  }
}

// ---- 4. pair rows ----------------------------------------------------------------------------------------------------------
// The row front of es_rows_body.  Per entry ONE shift lookup, distance and pair function, then pot_c += q_oc v for every channel
// and ONE force weight w = (sum_c q_ac q_oc) v'/d, which the pair force and the role-i cell partial use.
//   row_out[(C + 3) a + c]     = scale sum_e q_oc v_SR(d_e)                               (scale = 1, or 1/2 for a full list; both roles)
//   row_out[(C + 3) a + C + n] = scale sum_e (sum_c q_ac q_oc) v_SR'(d_e)/d_e (u_e)_n     (= the pair force on a)
//   cell_part[9 b + 3 m + n]   = scale sum over the role-i entries of the rows of block b of S_m w (u_e)_n     (CELL, float64)
template <typename T, int CAP, int PFAST, bool CELL>
__device__ __forceinline__ void ec_rows_body(const SRPot& sp, const FastRS& cf, int C, int64_t N, int64_t blk,
                                             const int* __restrict__ row_ptr, const int* __restrict__ ent32,
                                             const AtomRecord<T>* __restrict__ rec, const T* __restrict__ q, const T* __restrict__ cell,
                                             T scale, T* __restrict__ row_out, double* __restrict__ cell_part) {
  __shared__ AtomRecord<T> shift_tab[kShiftTableSize];
  __shared__ double red[kStepWaves][9];
  step_fill_shift_table(shift_tab, cell);
  __syncthreads();
  const T c_inv2s2 = T(cf.inv_2s2), c1 = T(cf.c1), cpref = T(cf.pref);
  const StepRow row = step_row(N, blk, row_ptr);
  const AtomRecord<T> pa = rec[row.a];
  T qa[CAP], pot[CAP];
  ec_charges<T, CAP>(q, row.a, C, qa);
#pragma unroll
  for (int c = 0; c < CAP; ++c) pot[c] = T(0);
  T fx = T(0), fy = T(0), fz = T(0);
  T w00 = T(0), w01 = T(0), w02 = T(0), w10 = T(0), w11 = T(0), w12 = T(0), w20 = T(0), w21 = T(0), w22 = T(0);
  for (int base = row.beg; base < row.end; base += 16) {
    const int e = base + row.sub;
    const StepEntry en = step_entry(ent32, e, row);
    const AtomRecord<T> po = rec[en.o];
    T qo[CAP];
    ec_charges<T, CAP>(q, int64_t(en.o), C, qo);
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
      T qq = T(0);
#pragma unroll
      for (int c = 0; c < CAP; ++c) {
        pot[c] += qo[c] * v;  // (a spare channel adds zeros to a sum nobody reads)
        if (c < C) qq += qa[c] * qo[c];
      }
      const T w = qq * dvd;
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
  T* o = row_out + (C + 3) * row.a;
  const bool writer = row.sub == 0 && row.valid;
#pragma unroll
  for (int c = 0; c < CAP; ++c)
    if (c < C) {
      const T s = row_sum(pot[c]);
      if (writer) o[c] = scale * s;
    }
  fx = row_sum(fx), fy = row_sum(fy), fz = row_sum(fz);
  if (writer) o[C] = scale * fx, o[C + 1] = scale * fy, o[C + 2] = scale * fz;
  if (CELL) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double s0 = wave_sum(double(w00)), s1 = wave_sum(double(w01)), s2 = wave_sum(double(w02));
    const double s3 = wave_sum(double(w10)), s4 = wave_sum(double(w11)), s5 = wave_sum(double(w12));
    const double s6 = wave_sum(double(w20)), s7 = wave_sum(double(w21)), s8 = wave_sum(double(w22));
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

// ---- 5. per-k cell gradient: 32 lanes per k-vector, records and charges streamed through LDS ---------------------------------
// gk = dE_raw/dk = dG |S|^2 k + G sum_j r_j (c A_s - s A_c),  A_s = sum_c q_jc S_s^c, A_c likewise,  |S|^2 = sum_c (S_c^c^2 + S_s^c^2),
// E_raw = 1/2 sum G |S|^2;  k_part: the ten partials per block of es_cellk_body
template <typename T, int CAP>
__device__ __forceinline__ void ec_cellk_body(int C, int64_t N, int64_t K, int64_t blk, const AtomRecord<T>* __restrict__ rec,
                                              const T* __restrict__ q, const T* __restrict__ kvec, const T* __restrict__ G,
                                              const T* __restrict__ dG, const T* __restrict__ Sc, const T* __restrict__ Ss,
                                              double* __restrict__ k_part) {
  __shared__ AtomRecord<T> sr[kStepTile];
  __shared__ T sq[CAP][kStepTile];
  __shared__ double red[kStepKPerBlock][kStepCellK];
  const int al = threadIdx.x % kStepKLanes, kl = threadIdx.x / kStepKLanes;
  const int64_t k = blk * kStepKPerBlock + kl;
  const bool live = k < K && (G[k] != T(0) || dG[k] != T(0));
  const int64_t kc = k < K ? k : 0;
  const T kx = kvec[3 * kc], ky = kvec[3 * kc + 1], kz = kvec[3 * kc + 2];
  T lSc[CAP], lSs[CAP];
#pragma unroll
  for (int c = 0; c < CAP; ++c) {
    lSc[c] = c < C ? Sc[c * K + kc] : T(0);
    lSs[c] = c < C ? Ss[c * K + kc] : T(0);
  }
  T ax = T(0), ay = T(0), az = T(0);
  for (int64_t base = 0; base < N; base += kStepTile) {
    const int n = int(min<int64_t>(kStepTile, N - base));
    __syncthreads();
    ec_stage_tile<T, CAP>(C, base, n, rec, q, sr, sq);
    __syncthreads();
    if (live)
      for (int i = al; i < n; i += kStepKLanes) {
        const AtomRecord<T> r = sr[i];
        T s, co;
        dipole_phase3(kx, ky, kz, r.x, r.y, r.z, s, co);
        T a_s = T(0), a_c = T(0);
#pragma unroll
        for (int c = 0; c < CAP; ++c)
          if (c < C) {
            const T qv = sq[c][i];
            a_s += qv * lSs[c];
            a_c += qv * lSc[c];
          }
        const T b = co * a_s - s * a_c;
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
      double s2 = 0.0;
#pragma unroll
      for (int c = 0; c < CAP; ++c)
        if (c < C) s2 += double(lSc[c]) * double(lSc[c]) + double(lSs[c]) * double(lSs[c]);
      const double gk = double(G[kc]), d = double(dG[kc]) * s2;
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
    for (int qq = 0; qq < kStepKPerBlock; ++qq) s += red[qq][threadIdx.x];
    k_part[kStepCellK * blk + threadIdx.x] = s;
  }
}

// ---- 6. finish -----------------------------------------------------------------------------------------------------------
// 16 lanes per atom over the slices, as es_finish_body.  Per atom and channel d_c = (phi_c / V - self q_ac - 2 bg Q_c / V) + pot_c
// goes to grad_q[a C + c]; the force is the pair force minus the three bracket sums over V; e_part: 1/2 sum_c q_ac d_c per block.
template <typename T, int CAP>
__device__ __forceinline__ void ec_finish_body(int C, int64_t N, int n_slices, int64_t blk, T self_c, double two_bg,
                                               const double* __restrict__ geom, const T* __restrict__ q, const T* __restrict__ part,
                                               const T* __restrict__ row_out, const double* __restrict__ q_part, int64_t n_q_blocks,
                                               T* __restrict__ forces, T* __restrict__ grad_q, double* __restrict__ e_part) {
  __shared__ double red[kStepWaves];
  const double inv_vol_d = geom[9];
  const T inv_vol = T(inv_vol_d);
  T bg_term[CAP];
#pragma unroll
  for (int c = 0; c < CAP; ++c) {
    bg_term[c] = T(0);
    if (two_bg != 0.0 && c < C) {  // (uniform) the same fixed order in every block
      const double Q = step_strided_sum(q_part, n_q_blocks, C, c, red);
      bg_term[c] = T(two_bg * Q * inv_vol_d);
    }
  }
  const int sub = threadIdx.x % 16;
  const int64_t a = blk * kStepRowsPerBlock + threadIdx.x / 16;
  const bool valid = a < N;
  T phi[CAP];
#pragma unroll
  for (int c = 0; c < CAP; ++c) phi[c] = T(0);
  T b0 = T(0), b1 = T(0), b2 = T(0);
  if (valid)
    for (int s = sub; s < n_slices; s += 16) {
      const T* __restrict__ p = part + (int64_t(s) * N + a) * (C + 3);
#pragma unroll
      for (int c = 0; c < CAP; ++c)
        if (c < C) phi[c] += p[c];
      b0 += p[C], b1 += p[C + 1], b2 += p[C + 2];
    }
#pragma unroll
  for (int c = 0; c < CAP; ++c)
    if (c < C) phi[c] = row_sum(phi[c]);
  b0 = row_sum(b0), b1 = row_sum(b1), b2 = row_sum(b2);
  double e = 0.0;
  if (valid && sub == 0) {
    const T* __restrict__ r = row_out + (C + 3) * a;
#pragma unroll
    for (int c = 0; c < CAP; ++c)
      if (c < C) {
        const T qa = q[a * C + c];
        const T d = ((inv_vol * phi[c] - self_c * qa) - bg_term[c]) + r[c];
        grad_q[a * C + c] = d;
        e += 0.5 * double(qa) * double(d);
      }
    forces[3 * a] = r[C] - inv_vol * b0;
    forces[3 * a + 1] = r[C + 1] - inv_vol * b1;
    forces[3 * a + 2] = r[C + 2] - inv_vol * b2;
  }
  e = block_sum<kStepWaves>(e, red);
  if (threadIdx.x == 0) e_part[blk] = e;
}

// ---- 7. final: one block per system ---------------------------------------------------------------------------------------
// es_final_body with the background of the cell gradient per channel: (E_k - bg sum_c Q_c^2) / V, NOT (sum_c Q_c)^2 -- the
// channels do not see each other's background
template <typename T, bool CELL>
__device__ __forceinline__ void ec_final_body(int C, int64_t n_e_blocks, const double* __restrict__ e_part, T* __restrict__ energy,
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
    double q2 = 0.0;
    for (int c = 0; c < C; ++c) {  // (uniform)
      const double s = step_strided_sum(q_part, n_q_blocks, C, c, red);
      q2 += s * s;
    }
    if (threadIdx.x == 0) tot[9 + kStepCellK] = q2;
    __syncthreads();
    if (threadIdx.x < 9) {
      const int m = threadIdx.x / 3, n = threadIdx.x % 3;
      const double* Wr = tot;
      const double* Wk = tot + 9;
      const double Ek = tot[9 + 9], Q2 = tot[9 + kStepCellK], inv_vol = geom[9];
      const double e_v = inv_vol * (Ek - bg * Q2);  // what scales with 1/V
      double chain = 0.0;
      for (int a = 0; a < 3; ++a) chain += geom[3 * a + m] * Wk[3 * a + n];
      grad_cell[3 * m + n] = bad ? T(NAN) : T(Wr[3 * m + n] - inv_vol * chain - e_v * geom[3 * n + m]);
    }
  }
}

}  // namespace mipme

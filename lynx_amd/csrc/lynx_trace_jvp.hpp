// gfx950 kernels of the beam trace's FORWARD-mode pass: the tangents of the beam moments at EVERY point of a lattice
// along D directions in parameter space (lynx_track_moments_along_forward, lynx_track_particles_along_forward).
// Included only by lynx_hip.hip, behind lynx_trace_grad.hpp.
//
// The reverse pass (lynx_trace_grad.hpp) answers one scalar loss and gives its gradient with respect to every parameter;
// this is the other shape: few parameters, every output -- the orbit response matrix (d centroid at every BPM / d angle of
// every corrector), the Jacobian of residuals of a least-squares matching, "how does beta_x at every point move when Q3 is
// turned".  The trace's program has every leaf element as a step of its own (LYNX_STEP_FLAG_RAW: S = E, P = E + 1), and
// without a cavity step every element is an affine map of the 7-vector, so for a direction d
//
//   mu_dot[0] = 0, C_dot[0] = 0
//   for k = 1 .. S:
//     Mdot = sum over the direction's entries at element k - 1 of weight . dM_{k-1}/d(parameter or energy)   (none for most k)
//     mu_dot[k] = M mu_dot[k-1] + Mdot mu[k-1]
//     C_dot[k]  = M C_dot[k-1] M^T + X + X^T,   X = Mdot C[k-1] M^T
//
// with mu[k], C[k] READ from the forward trace, as k_trace_moments_bwd reads them, and M the step's row of the trace's
// table.  The mean and the biased covariance of a ParticleBeam obey the same recursion exactly (the head of
// lynx_trace_grad.hpp), so its tangents come from the moment records and no pass over the particles is made.
//
// A direction is a short list of entries (leaf, parameter row 0 .. 7 or kGradParams for the step energy, weight), the
// whole set in CSR form -- dir_start [D + 1], dir_leaf [n], dir_row [n], dir_weight [n] float64 -- with the entries of one
// direction ordered by leaf (the host orders them).  That covers an element object that occurs several times, RBend's
// `angle` (which feeds e1 and e2 with weight 1/2), the two rows of a vector parameter and the incoming energy (one
// kGradParams entry per leaf, weight 1).
//
// The sweep's own arithmetic is float64 for every lattice dtype, for the reason the head of lynx_trace_grad.hpp gives: the
// tangent of a Twiss value is the contraction of C_dot with -(beta / 2 eps) C^-1 and its like, which cancels (1 +
// alpha^2)-fold.  The maps and dM are the lattice's dtype (the builders'); the states are read as the trace left them.
//
//   k_trace_tangent_maps      one thread per (sample, entry): weight . dM of that entry's element along that entry's row by
//                             dual evaluation (step 3 of build_bwd_sample), 49 float64 to [B][n][49]
//   k_trace_records_to_moments   ParticleBeam: moment records [B][P][36] float64 -> mu, C of the sweep
//                             (k_trace_records_to_states without its cotangent half)
//   k_trace_moments_jvp       the sweep, one wave per (sample, direction)
// and through gaining cavities (lynx_track_moments_along_forward_cavities; the section in front of
// k_trace_energy_tangents):
//   k_trace_energy_tangents   one thread per (sample, direction): the tangent of the beam energy at every point
//   k_trace_tangent_rows      k_trace_tangent_maps at the step's own energy, with the 8 cavity coefficients: [B][n][64]
//   k_trace_moments_jvp_kicks the same sweep with the tangent of the cavity branch behind a gaining cavity's products
#pragma once

#include "lynx_device.hpp"
#include "lynx_grad.hpp"
#include "lynx_trace.hpp"

namespace lynx {

// The directions on the device, one block: int32 dir_start [D + 1] | dir_leaf [n] | dir_row [n], then (8-aligned) float64
// dir_weight [n].
struct TraceDirections {
  const int32_t* start;
  const int32_t* leaf;
  const int32_t* row;
  const double* weight;
  int32_t count;    // D
  int32_t entries;  // n
};

// ---------------------------------------------------------------------------------------
// k_trace_tangent_maps: grid = ceil(B n / 64), 64 threads, thread = (sample, entry).  What step 3 of build_bwd_sample does
// per (element, parameter): the element's builder on dual numbers with the tangent seed on the entry's row (row ==
// kGradParams: on the step energy), through the 16 entries of class U in registers where the kind has that structure
// (build_entries_u: an entry outside the pattern has derivative zero) and through build_element otherwise.  The program
// has no cavity step (refused by the host), so the energy at every step is the incoming one -- what the trace's energy
// record holds at every point.  A kind without parameters (identity, custom map) has no derivative: zeros.  The
// derivative conventions are the builders' (lynx_dual.hpp).  Every thread writes its 49 cells.
// (Compiled for k_build_bwd's waves per SIMD, not for speed of its own: the dual-number builders are out-of-line functions
// that the two kernels SHARE, and the register budget they are compiled for is the loosest of their callers' -- without the
// attribute here k_build_bwd<float> went from 72 registers and six waves to 132 and three, and BASELINE config 5's reverse
// pass from 2.00 to 2.08 ms.)
// ---------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(sizeof(T) == 4 ? 7 : 1))) void k_trace_tangent_maps(LatticeDev lat, const T* __restrict__ energy_in, TraceDirections dirs,
                                                           double* __restrict__ mdot /* [B][n][49] */) {
  const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
  const int64_t n = dirs.entries;
  if (t >= lat.batch * n) return;
  const int64_t b = t / n;
  const int q = (int)(t - b * n);
  const int e = dirs.leaf[q], pidx = dirs.row[q];
  const double w = dirs.weight[q];
  double* out = mdot + t * 49;
  const lynx_elem el = lat.elems[e];
  const int np = bwd_kind_params_dev(el.kind);
  const bool energy_task = pidx == kGradParams;
  if (np == 0) {
    for (int c = 0; c < 49; ++c) out[c] = 0.0;
    return;
  }
  const T* p = static_cast<const T*>(lat.pool) + el.param_offset + b * (int64_t)el.batch_stride;
  Dual<T> dp[8];
  for (int k = 0; k < 8; ++k) dp[k] = Dual<T>(k < np ? p[k] : T(0), (k == pidx) ? T(1) : T(0));
  const Dual<T> de(energy_in[b], energy_task ? T(1) : T(0));
  Dual<T> m16[16];
  if (build_entries_u<Dual<T>>(el.kind, el.flags, dp, de, m16, nullptr)) {
    for (int c = 0; c < 49; ++c) out[c] = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) out[unit_entry_u(k)] = w * (double)m16[k].d;
  } else {
    Dual<T> dM[49];
    build_element<Dual<T>>(el.kind, el.flags, dp, de, dM, nullptr);
    for (int c = 0; c < 49; ++c) out[c] = w * (double)dM[c].d;
  }
}

// ---------------------------------------------------------------------------------------
// Through gaining cavities (lynx_track_moments_along_forward_cavities, a ParameterBeam).  Two things change.  The energy
// that enters step k is E_in + the sum of V cos(phi) over the gaining cavities in front of it, so a direction carries an
// energy tangent e_dot[k] -- its seed at point 0 (1 for the incoming energy), + w cos(phi) at a gaining cavity for a
// voltage entry, - w V sin(phi) pi/180 for a phase entry: the forward image of step 4 of build_bwd_sample -- and an
// entry on the energy's row contributes weight . e_dot[leaf] . dR/dE.  And behind the products of a gaining cavity comes
// the tangent of moment_cavity_branch, which needs the tangents of the step's 8 coefficients beside those of its map: an
// entry's tangent is the row R = map | coefficients, 64 wide.
//
// k_trace_energy_tangents: grid = ceil(B D / 64), thread = (sample, direction): e_dot at every point, [B][D][P], every
// cell written.  The entries of a direction are ordered by leaf, so one walk over the points consumes them in order.
// Whether a cavity gains is what the table says of this sample's build (LYNX_FLAGS_OFFSET), as everywhere in the trace.
// ---------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(64) void k_trace_energy_tangents(LatticeDev lat, const T* __restrict__ steps, TraceDirections dirs,
                                                              const double* __restrict__ seed /* [D] */,
                                                              double* __restrict__ energy_dot /* [B][D][P] */) {
  const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
  const int D = dirs.count, S = lat.n_steps, P = S + 1;
  if (t >= lat.batch * D) return;
  const int64_t b = t / D;
  const int d = (int)(t - b * D);
  const T* pool = static_cast<const T*>(lat.pool);
  double* out = energy_dot + t * P;
  int q = dirs.start[d];
  const int q_end = dirs.start[d + 1];
  double e = seed[d];
  for (int s = 0; s <= S; ++s) {
    out[s] = e;
    if (s == S) break;
    for (; q < q_end && dirs.leaf[q] == s; ++q) {
      const int row = dirs.row[q];
      if (row != 1 && row != 2) continue;  // (of a cavity: voltage, phase)
      const int desc = (int)steps[(b * S + s) * LYNX_STEP_STRIDE + LYNX_FLAGS_OFFSET];
      if (((desc >> LYNX_DESC_KIND_SHIFT) & 3) != LYNX_STEP_CAVITY || !(desc & LYNX_FLAG_CAV_GAIN)) continue;
      const lynx_elem el = lat.elems[lat.steps[s].first];
      const T* p = pool + el.param_offset + b * (int64_t)el.batch_stride;
      const double phi = (double)p[2] * (LYNX_PI / 180.0);
      e += row == 1 ? dirs.weight[q] * cos(phi) : -dirs.weight[q] * (double)p[1] * sin(phi) * (LYNX_PI / 180.0);
    }
  }
}

// ---------------------------------------------------------------------------------------
// k_trace_tangent_rows: k_trace_tangent_maps with the step's own entering energy as the value of the dual (`energy`
// [B][P]: what k_trace_energies writes, the build's own sums), the coefficient output of the builders as step 3 of
// build_bwd_sample asks for it, and weight . e_dot[leaf] as the factor of an entry on the energy's row (`energy_dot`:
// k_trace_energy_tangents, launched in front; the entry's direction by bisection of dir_start).  64 float64 per
// (sample, entry): 49 map entries, 8 coefficients, zeros.  Every thread writes its 64 cells.  The waves per SIMD: see
// k_trace_tangent_maps -- the dual builders are k_build_bwd's, too.
// ---------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(sizeof(T) == 4 ? 7 : 1))) void k_trace_tangent_rows(LatticeDev lat, const T* __restrict__ energy /* [B][P] */, TraceDirections dirs,
                                                           const double* __restrict__ energy_dot /* [B][D][P] */,
                                                           double* __restrict__ rdot /* [B][n][64] */) {
  const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
  const int64_t n = dirs.entries;
  if (t >= lat.batch * n) return;
  const int64_t b = t / n;
  const int q = (int)(t - b * n);
  const int e = dirs.leaf[q], pidx = dirs.row[q];
  const int P = lat.n_steps + 1;
  double* out = rdot + t * LYNX_STEP_STRIDE;
  for (int c = 0; c < LYNX_STEP_STRIDE; ++c) out[c] = 0.0;
  const lynx_elem el = lat.elems[e];
  const int np = bwd_kind_params_dev(el.kind);
  if (np == 0) return;
  const bool energy_task = pidx == kGradParams;
  double w = dirs.weight[q];
  if (energy_task) {
    int lo = 0, hi = dirs.count;  // the last direction whose entries start at or in front of q
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (dirs.start[mid] <= q) lo = mid;
      else hi = mid;
    }
    w *= energy_dot[(b * dirs.count + lo) * P + e];
  }
  const T* p = static_cast<const T*>(lat.pool) + el.param_offset + b * (int64_t)el.batch_stride;
  Dual<T> dp[8];
  for (int k = 0; k < 8; ++k) dp[k] = Dual<T>(k < np ? p[k] : T(0), (k == pidx) ? T(1) : T(0));
  const Dual<T> de(energy[b * P + e], energy_task ? T(1) : T(0));
  const bool cav_step = lat.steps[e].kind == LYNX_STEP_CAVITY;
  Dual<T> dC[8];
  for (int k = 0; k < 8; ++k) dC[k] = Dual<T>(T(0));
  Dual<T> m16[16];
  if (build_entries_u<Dual<T>>(el.kind, el.flags, dp, de, m16, cav_step ? dC : nullptr)) {
#pragma unroll
    for (int k = 0; k < 16; ++k) out[unit_entry_u(k)] = w * (double)m16[k].d;
  } else {
    Dual<T> dM[49];
    build_element<Dual<T>>(el.kind, el.flags, dp, de, dM, cav_step ? dC : nullptr);
    for (int c = 0; c < 49; ++c) out[c] = w * (double)dM[c].d;
  }
  if (cav_step)
    for (int k = 0; k < 8; ++k) out[LYNX_COEF_OFFSET + k] = w * (double)dC[k].d;
}

// ---------------------------------------------------------------------------------------
// jvp_cavity_branch: the tangent of moment_cavity_branch (lynx_device.hpp), lane 0 of a gaining cavity step behind the
// linear products.  s_m, s_d: the step's row and its tangent (map | coefficients); s_mu, s_c: the state that ENTERED the
// step; in_d: the tangents that entered it (mu_dot[4], mu_dot[5], C_dot[4][4], [4][5], [5][5]); s_md, s_cd: the linear
// step's tangents, which the branch's entries go over.  With a = -z4 c2 + c3:
//   mu'[5] = z5 c0 + c1 (cos a - c4),   mu'[4] += c5 z5^2 + c6 z4 z5 + c7 z4^2,   C'[5][5] = c55,
//   C'[4][4] = C'[4][5] = C'[5][4] = c5 c55^2 + c6 c45 c55 + c7 c44^2
// The differences cos a - cos phi and sin a - sin phi are formed as kick_cotangents forms them (sin_cosm1 of d = a - phi
// and the addition theorems), and the phase's tangent enters as -c1 (sin a - sin phi) c3_dot -- d/dc3 and the path through
// c4 = cos(phi) in one term, never two that cancel; the tangent of c4 itself is not read.
// ---------------------------------------------------------------------------------------
template <typename A>
__device__ __forceinline__ void jvp_cavity_branch(const A* s_m, const A* s_d, const A* s_mu, const A* s_c, const A (&in_d)[5],
                                                  A* s_md, A* s_cd) {
  const A* c = s_m + LYNX_COEF_OFFSET;
  const A* cdot = s_d + LYNX_COEF_OFFSET;
  const A z4 = s_mu[4], z5 = s_mu[5], c44 = s_c[4 * 7 + 4], c45 = s_c[4 * 7 + 5], c55 = s_c[5 * 7 + 5];
  const A zd4 = in_d[0], zd5 = in_d[1], cd44 = in_d[2], cd45 = in_d[3], cd55 = in_d[4];
  A sphi, cphi, sd, cm1;
  phase_sincos(c[LYNX_C_PHI], sphi, cphi);
  sin_cosm1(-z4 * c[LYNX_C_BK], sd, cm1);
  const A dsin = fma(sd, cphi, cm1 * sphi);   // sin(a) - sin(phi)
  const A dcos = fma(sd, -sphi, cm1 * cphi);  // cos(a) - cos(phi)
  const A sa = dsin + sphi;
  const A ad = -zd4 * c[LYNX_C_BK] - z4 * cdot[LYNX_C_BK];  // a_dot without the phase's own term
  s_md[5] = zd5 * c[LYNX_C_DSCALE] + z5 * cdot[LYNX_C_DSCALE] + cdot[LYNX_C_DKICK] * dcos -
            c[LYNX_C_DKICK] * (sa * ad + dsin * cdot[LYNX_C_PHI]);
  s_md[4] += cdot[LYNX_C_T566] * (z5 * z5) + A(2) * c[LYNX_C_T566] * z5 * zd5 + cdot[LYNX_C_T556] * z4 * z5 +
             c[LYNX_C_T556] * (zd4 * z5 + z4 * zd5) + cdot[LYNX_C_T555] * (z4 * z4) + A(2) * c[LYNX_C_T555] * z4 * zd4;
  const A v = cdot[LYNX_C_T566] * (c55 * c55) + A(2) * c[LYNX_C_T566] * c55 * cd55 + cdot[LYNX_C_T556] * c45 * c55 +
              c[LYNX_C_T556] * (cd45 * c55 + c45 * cd55) + cdot[LYNX_C_T555] * (c44 * c44) + A(2) * c[LYNX_C_T555] * c44 * cd44;
  s_cd[5 * 7 + 5] = cd55;
  s_cd[4 * 7 + 4] = v;
  s_cd[4 * 7 + 5] = v;
  s_cd[5 * 7 + 4] = v;
}

// ---------------------------------------------------------------------------------------
// k_trace_records_to_moments: grid = B * P, 64 threads.  Record layout of LYNX_MOMENT_STRIDE: [0..6] mean, [7..27] the
// upper triangle of the biased covariance; the 7th row and column of C are zero (the 7th coordinate is 1 for every
// particle).
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_trace_records_to_moments(const double* __restrict__ trace_fwd, double* __restrict__ mu,
                                                                 double* __restrict__ cov) {
  const int64_t p = blockIdx.x;
  const int lane = threadIdx.x;
  const double* rec = trace_fwd + p * LYNX_MOMENT_STRIDE;
  if (lane < 7) mu[p * 7 + lane] = lane < 6 ? rec[lane] : 1.0;
  if (lane < 49) {
    const int i = lane / 7, j = lane - i * 7;
    double c = 0.0;
    if (i < 6 && j < 6) {
      const int r = i < j ? i : j, q = i < j ? j : i;
      c = rec[7 + r * 6 - (r * (r - 1)) / 2 + (q - r)];
    }
    cov[p * 49 + lane] = c;
  }
}

// ---------------------------------------------------------------------------------------
// k_trace_moments_jvp: grid = B * D, one wave per (sample, direction), 49 lanes busy (lane = entry i * 7 + j; lanes 0 .. 6
// also own mu_dot).  Per step, with the state that ENTERS it (point s of the forward trace), its row M and -- if the
// direction has an entry at this leaf -- Mdot, the sum of the direction's entries there in entry order:
//   row, state and Mdot from registers to LDS                                 | barrier
//   Y = C_dot M^T,  Z = C M^T (with Mdot only)                                | barrier
//   mu_dot' = M mu_dot (+ Mdot mu),   C_dot' = M Y (+ X + X^T, X = Mdot Z: a lane forms its own X_ij and X_ji)
//   every read of mu_dot, C_dot                                              | barrier
//   mu_dot', C_dot' over them and out to point s + 1                         (the next step's first barrier follows)
// A step WITHOUT an entry of the direction skips the Mdot terms altogether -- it does not multiply by a zero matrix, so a
// NaN map or state elsewhere does not reach it.  The 7th coordinate is the constant 1: entry 6 of mu_dot and row and
// column 6 of C_dot are written as the exact zeros they are, at every point.  What step s + 1 needs from memory (row,
// state, the entries' Mdot: independent of the sweep) is fetched while step s is worked on -- the sweep is a chain of small
// dependent products, and a wave would otherwise wait for memory once per step.  One lane owns every cell it writes, the
// sums run in a fixed order, no atomics: the same call returns the same bits.
// ---------------------------------------------------------------------------------------
template <typename T, typename ST, bool KICK>
__device__ __forceinline__ void trace_moments_jvp_wave(int S, const TraceDirections& dirs, const T* __restrict__ steps,
                                                       const ST* __restrict__ mu_trace, const ST* __restrict__ cov_trace,
                                                       const double* __restrict__ mdot /* [B][n][kRow] */,
                                                       double* __restrict__ mu_dot /* [B][D][P][7] */,
                                                       double* __restrict__ cov_dot /* [B][D][P][49] */) {
  using A = double;  // the sweep's own arithmetic, whatever the lattice's dtype (see the head of this file)
  constexpr int kRow = KICK ? LYNX_STEP_STRIDE : 49;  // an entry's tangent: the map (KICK: and the 8 coefficients behind it)
  __shared__ A s_m[64], s_mu[8], s_c[49], s_d[kRow], s_md[8], s_cd[49], s_y[49], s_z[49];
  const int D = dirs.count;
  const int64_t b = blockIdx.x / D;
  const int d = (int)(blockIdx.x - b * D);
  const int lane = threadIdx.x;
  const int cl = lane < 49 ? lane : 48, l7 = lane < 7 ? lane : 6;
  const int i = cl / 7, j = cl % 7;
  const int P = S + 1;
  const bool constant = i == 6 || j == 6;  // the 7th coordinate: no tangent
  const T* g_steps = steps + b * (int64_t)S * LYNX_STEP_STRIDE;
  const ST* g_mu = mu_trace + b * (int64_t)P * 7;
  const ST* g_c = cov_trace + b * (int64_t)P * 49;
  const double* g_d = mdot + b * (int64_t)dirs.entries * kRow;
  double* o_mu = mu_dot + (b * D + d) * (int64_t)P * 7;
  double* o_c = cov_dot + (b * D + d) * (int64_t)P * 49;
  int q = dirs.start[d];
  const int q_end = dirs.start[d + 1];

  // point 0: no parameter reaches the incoming beam
  if (lane < 7) {
    s_md[lane] = A(0);
    o_mu[lane] = A(0);
  }
  if (lane < 49) {
    s_cd[lane] = A(0);
    o_c[lane] = A(0);
  }
  // (clamped lanes read a valid cell twice and use nothing of it)
  A n_m = A(0), n_mu = A(0), n_c = A(0), n_d = A(0);
  bool n_has = false;
  int at = q < q_end ? dirs.leaf[q] : -1;  // the leaf of the direction's next entry (uniform)
  const auto fetch = [&](int s) {
    n_m = (A)g_steps[(int64_t)s * LYNX_STEP_STRIDE + lane];
    n_mu = (A)g_mu[(int64_t)s * 7 + l7];
    n_c = (A)g_c[(int64_t)s * 49 + cl];
    n_d = A(0);
    n_has = false;
    while (at == s) {  // (uniform)
      n_d += g_d[(int64_t)q * kRow + (KICK ? lane : cl)];
      n_has = true;
      ++q;
      at = q < q_end ? dirs.leaf[q] : -1;
    }
  };
  if (S > 0) fetch(0);
  for (int s = 0; s < S; ++s) {
    s_m[lane] = n_m;
    if (lane < 7) s_mu[lane] = n_mu;
    if (lane < 49) {
      s_c[lane] = n_c;
      s_d[lane] = n_d;
    }
    if constexpr (KICK) {
      if (lane >= 49) s_d[lane] = n_d;  // the coefficients' tangents (zeros where the direction has no entry here)
    }
    const bool has = n_has;
    if (s + 1 < S) fetch(s + 1);
    __syncthreads();
    bool kick = false;                                               // (uniform) a gaining cavity: its branch follows the products
    A in_d[5] = {A(0), A(0), A(0), A(0), A(0)};                      // ... on the tangents that ENTER the step, parked here
    if constexpr (KICK) {
      const int desc = (int)s_m[LYNX_FLAGS_OFFSET];
      kick = ((desc >> LYNX_DESC_KIND_SHIFT) & 3) == LYNX_STEP_CAVITY && (desc & LYNX_FLAG_CAV_GAIN);
      if (kick) {
        in_d[0] = s_md[4], in_d[1] = s_md[5];
        in_d[2] = s_cd[4 * 7 + 4], in_d[3] = s_cd[4 * 7 + 5], in_d[4] = s_cd[5 * 7 + 5];
      }
    }
    A y = s_cd[i * 7] * s_m[j * 7], z = A(0);  // Y = C_dot M^T
#pragma unroll
    for (int k = 1; k < 7; ++k) y = fma(s_cd[i * 7 + k], s_m[j * 7 + k], y);
    if (has) {
      z = s_c[i * 7] * s_m[j * 7];  // Z = C M^T
#pragma unroll
      for (int k = 1; k < 7; ++k) z = fma(s_c[i * 7 + k], s_m[j * 7 + k], z);
    }
    if (lane < 49) {
      s_y[lane] = y;
      s_z[lane] = z;
    }
    __syncthreads();
    A cd = s_m[i * 7] * s_y[j];  // M Y
#pragma unroll
    for (int k = 1; k < 7; ++k) cd = fma(s_m[i * 7 + k], s_y[k * 7 + j], cd);
    A md = s_m[l7 * 7] * s_md[0];  // M mu_dot
#pragma unroll
    for (int k = 1; k < 7; ++k) md = fma(s_m[l7 * 7 + k], s_md[k], md);
    if (has) {
      A x = s_d[i * 7] * s_z[j], xt = s_d[j * 7] * s_z[i];  // X_ij, X_ji of X = Mdot Z
#pragma unroll
      for (int k = 1; k < 7; ++k) {
        x = fma(s_d[i * 7 + k], s_z[k * 7 + j], x);
        xt = fma(s_d[j * 7 + k], s_z[k * 7 + i], xt);
      }
      cd += x + xt;
      A dm = s_d[l7 * 7] * s_mu[0];  // Mdot mu
#pragma unroll
      for (int k = 1; k < 7; ++k) dm = fma(s_d[l7 * 7 + k], s_mu[k], dm);
      md += dm;
    }
    if (constant) cd = A(0);
    if (l7 == 6) md = A(0);
    __syncthreads();
    if constexpr (KICK) {
      if (kick) {  // moment_step_wave's barriers 3 and 4: the linear tangents written | lane 0's entries over them | their reads
        if (lane < 7) s_md[lane] = md;
        if (lane < 49) s_cd[lane] = cd;
        __syncthreads();
        if (lane == 0) jvp_cavity_branch<A>(s_m, s_d, s_mu, s_c, in_d, s_md, s_cd);
        __syncthreads();
        md = s_md[l7];
        cd = s_cd[cl];
      }
    }
    if (lane < 7) {
      s_md[lane] = md;
      o_mu[(int64_t)(s + 1) * 7 + lane] = md;
    }
    if (lane < 49) {
      s_cd[lane] = cd;
      o_c[(int64_t)(s + 1) * 49 + lane] = cd;
    }
    // (no barrier here: what the next step writes first -- row, state, Mdot -- was last read in front of the barrier above,
    // and its own first barrier stands between these writes of mu_dot, C_dot and their reads)
  }
}

template <typename T, typename ST>
__global__ __launch_bounds__(64) void k_trace_moments_jvp(int S, TraceDirections dirs, const T* __restrict__ steps,
                                                          const ST* __restrict__ mu_trace, const ST* __restrict__ cov_trace,
                                                          const double* __restrict__ mdot /* [B][n][49] */,
                                                          double* __restrict__ mu_dot /* [B][D][P][7] */,
                                                          double* __restrict__ cov_dot /* [B][D][P][49] */) {
  trace_moments_jvp_wave<T, ST, false>(S, dirs, steps, mu_trace, cov_trace, mdot, mu_dot, cov_dot);
}

// ... through gaining cavities (a ParameterBeam's states): the same body with the cavity branch's tangent behind the
// products, the entries' tangents 64 wide (k_trace_tangent_rows).
template <typename T>
__global__ __launch_bounds__(64) void k_trace_moments_jvp_kicks(int S, TraceDirections dirs, const T* __restrict__ steps,
                                                                const T* __restrict__ mu_trace, const T* __restrict__ cov_trace,
                                                                const double* __restrict__ rdot /* [B][n][64] */,
                                                                double* __restrict__ mu_dot /* [B][D][P][7] */,
                                                                double* __restrict__ cov_dot /* [B][D][P][49] */) {
  trace_moments_jvp_wave<T, T, true>(S, dirs, steps, mu_trace, cov_trace, rdot, mu_dot, cov_dot);
}

}  // namespace lynx

// gfx950 kernels of the beam trace's reverse pass: the gradient of any function of the beam moments at EVERY point of
// a lattice (lynx_track_moments_along_backward, lynx_track_particles_along_backward).  Included only by lynx_hip.hip,
// behind lynx_grad.hpp and lynx_trace.hpp.
//
// For a lattice without a kicking cavity every element is an affine map of the 7-vector, so the mean and the biased
// covariance of a ParticleBeam obey the ParameterBeam's recursion exactly: mu_k = M_k mu_{k-1},
// C_k = M_k C_{k-1} M_k^T.  The gradient of a function of the moments at all points therefore needs no pass over the
// particles: it is the reverse sweep of the moment recursion with a cotangent injected at every point,
//
//   m = 0, G = 0
//   for k = S .. 1:                      (point k lies behind step k - 1)
//     m += mu_bar[k], G += cov_bar[k]
//     (active cavity: the direct terms and coefficient cotangents, sweep_kick)
//     T_bar[k-1] = m (x) mu[k-1] + (G M) C[k-1]^T + (G^T M) C[k-1]
//     m <- M^T m,  G <- M^T G M
//   grad_mu_in = m + mu_bar[0],  grad_cov_in = G + cov_bar[0]
//
// with mu[k], C[k] read from the forward trace.  T_bar leaves in the layout k_build_bwd consumes.  One step of the loop
// is sweep_kick and sweep_products of lynx_grad.hpp, the functions k_moments_bwd runs in the lattice's dtype; the
// recursion itself, where a kernel here needs it, is moment_step_wave of lynx_device.hpp.
//
// The sweep's own arithmetic is float64 for every lattice dtype.  The cotangent of a Twiss value carries
// -(beta / 2 eps) C^-1, and (G M) C^T then forms C^-1 C = 1 as gamma beta - alpha^2: a sum that cancels (1 + alpha^2)-fold
// (240-fold for a beam that enters a FODO channel with five times its matched beta, 5000-fold at thirty times).  In
// float32 that cancellation, carried through 128 steps, left gradients 5e-3 .. 0.3 from the float64 pass; the sweep is
// 49 lanes of small products per step and costs the same either way.  A ParticleBeam's states and cotangents stay the
// float64 they are in the records; a ParameterBeam's are read in the lattice's dtype.
//
//   k_trace_records_to_states   ParticleBeam: moment records and record cotangents [B][P][36] float64 -> mu, C, mu_bar,
//                               cov_bar of the sweep
//   k_trace_moments_bwd         the sweep, one wave per sample (sweep_kick, sweep_products in float64)
//   k_trace_energy_bwd          the cotangents of the beam energy at every point -> incoming energy and the gaining
//                               cavities' voltage and phase (adds into what k_build_bwd wrote)
//   k_trace_trajectories_bwd    the reverse sweep of CHOSEN particles' trajectories (lynx_track_particles_along_backward_
//                               trajectories): a cotangent on single coordinates at every point, through the kick as well
//   k_trace_moments_bwd_sets    a trace with losses (lynx_track_particles_along_backward_losses): per nested survivor
//                               set the recursion from the set's incoming moments (moment_step_wave) and the sweep over
//                               its own points (sweep_products), both in float64;
//                               k_trace_sum_sets adds the sets' T_bar in set order
#pragma once

#include "lynx_device.hpp"
#include "lynx_grad.hpp"
#include "lynx_trace.hpp"

namespace lynx {

// ---------------------------------------------------------------------------------------
// k_trace_records_to_states: grid = B * P, 64 threads.  Record layout of LYNX_MOMENT_STRIDE: [0..6] mean, [7..27] the
// upper triangle of the biased covariance.  A record cotangent counts an off-diagonal entry once (the convention of
// lynx_track_particles_backward): G_ii = c_ii, G_ij = G_ji = c_ij / 2.  The 7th row and column of C are zero (the 7th
// coordinate is 1 for every particle); the 7th column of cov_bar multiplies them, so it is zero as well.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_trace_records_to_states(const double* __restrict__ trace_fwd,
                                                                const double* __restrict__ grad_trace,
                                                                double* __restrict__ mu, double* __restrict__ cov,
                                                                double* __restrict__ mu_bar, double* __restrict__ cov_bar) {
  const int64_t p = blockIdx.x;
  const int lane = threadIdx.x;
  const double* rec = trace_fwd + p * LYNX_MOMENT_STRIDE;
  const double* g = grad_trace + p * LYNX_MOMENT_STRIDE;
  if (lane < 7) {
    mu[p * 7 + lane] = lane < 6 ? rec[lane] : 1.0;
    mu_bar[p * 7 + lane] = g[lane];
  }
  if (lane < 49) {
    const int i = lane / 7, j = lane - i * 7;
    double c = 0.0, cb = 0.0;
    if (i < 6 && j < 6) {
      const int r = i < j ? i : j, q = i < j ? j : i;
      const int t = 7 + r * 6 - (r * (r - 1)) / 2 + (q - r);
      c = rec[t];
      cb = i == j ? g[t] : 0.5 * g[t];
    }
    cov[p * 49 + lane] = c;
    cov_bar[p * 49 + lane] = cb;
  }
}

// ---------------------------------------------------------------------------------------
// k_trace_moments_bwd: grid = B, one wave per sample, 49 lanes busy (lane = entry i * 7 + j), every step by sweep_kick
// and sweep_products.  Nothing is recomputed and nothing parked: the state that ENTERS step s is point s of
// the forward trace.  The cotangent of point s + 1 is added BEFORE step s is reversed, so a cotangent on the entries an
// active cavity overwrites (mu[5], cov[4,4], cov[4,5], cov[5,4], cov[5,5]) goes through the kick's formulas, not
// through M.  What step s - 1 needs from memory (state, table row, cotangents: independent of the sweep) is fetched
// while step s is worked on -- the sweep is a chain of small dependent products, and a sample's wave would otherwise
// wait for memory once per step.  One lane owns every cell it writes, the sums run in a fixed order: the same call
// returns the same bits.
// ---------------------------------------------------------------------------------------
template <typename T, typename ST>
__global__ __launch_bounds__(64) void k_trace_moments_bwd(int S, const T* __restrict__ steps,
                                                          const ST* __restrict__ mu_trace, const ST* __restrict__ cov_trace,
                                                          const ST* __restrict__ mu_bar, const ST* __restrict__ cov_bar,
                                                          T* __restrict__ tbar, T* __restrict__ grad_mu_in,
                                                          T* __restrict__ grad_cov_in) {
  using A = double;  // the sweep's own arithmetic, whatever the lattice's dtype (see the head of this file)
  __shared__ A s_mu[8], s_c[49], s_x[49], s_y[49], s_g[49], s_mb[8], s_m[64], s_k[16];
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x;
  const int cl = lane < 49 ? lane : 48, l7 = lane < 7 ? lane : 6;
  const int i = cl / 7, j = cl % 7;
  const int P = S + 1;
  const T* g_steps = steps + b * (int64_t)S * LYNX_STEP_STRIDE;
  const ST* g_mu = mu_trace + b * (int64_t)P * 7;
  const ST* g_c = cov_trace + b * (int64_t)P * 49;
  const ST* g_mb = mu_bar + b * (int64_t)P * 7;
  const ST* g_cb = cov_bar + b * (int64_t)P * 49;

  if (lane < 7) s_mb[lane] = A(0);
  if (lane < 49) s_g[lane] = A(0);
  // (clamped lanes read a valid cell twice and use nothing of it)
  A n_mu = A(0), n_c = A(0), n_m = A(0), n_mb = g_mb[(int64_t)S * 7 + l7], n_cb = g_cb[(int64_t)S * 49 + cl];
  if (S > 0) {
    n_mu = g_mu[(int64_t)(S - 1) * 7 + l7];
    n_c = g_c[(int64_t)(S - 1) * 49 + cl];
    n_m = g_steps[(int64_t)(S - 1) * LYNX_STEP_STRIDE + lane];
  }
  __syncthreads();
  for (int s = S - 1; s >= 0; --s) {
    if (lane < 7) {
      s_mb[lane] += n_mb;  // cotangent of point s + 1
      s_mu[lane] = n_mu;   // state at point s
    }
    if (lane < 49) {
      s_g[lane] += n_cb;
      s_c[lane] = n_c;
    }
    s_m[lane] = n_m;
    if (lane < 16) s_k[lane] = A(0);
    n_mb = g_mb[(int64_t)s * 7 + l7];
    n_cb = g_cb[(int64_t)s * 49 + cl];
    if (s > 0) {
      n_mu = g_mu[(int64_t)(s - 1) * 7 + l7];
      n_c = g_c[(int64_t)(s - 1) * 49 + cl];
      n_m = g_steps[(int64_t)(s - 1) * LYNX_STEP_STRIDE + lane];
    }
    __syncthreads();
    const int desc = (int)s_m[LYNX_FLAGS_OFFSET];
    const bool kick = ((desc >> LYNX_DESC_KIND_SHIFT) & 3) == LYNX_STEP_CAVITY && (desc & LYNX_FLAG_CAV_GAIN);
    if (kick && lane == 0) sweep_kick<A>(s_m, s_mu, s_c, s_g, s_mb, s_k);
    __syncthreads();
    A tb, cb, mbn;
    sweep_products<A>(s_m, s_mu, s_c, s_g, s_mb, s_x, s_y, lane, i, j, tb, cb, mbn);
    T* tb_out = tbar + (b * S + s) * (int64_t)kGradStride;
    if (lane < 49) tb_out[lane] = tb;
    else if (lane < 57) tb_out[lane] = s_k[lane - 49];
    else tb_out[lane] = A(0);
    __syncthreads();
    if (lane < 49) s_g[lane] = cb;
    if (lane < 7) s_mb[lane] = mbn;
    __syncthreads();
    if (kick && lane == 0) {
      s_mb[4] += s_k[8];
      s_mb[5] += s_k[9];
      s_g[32] += s_k[10];
      s_g[33] += s_k[11];
      s_g[40] += s_k[12];
    }
    __syncthreads();
  }
  if (lane < 7) grad_mu_in[b * 7 + lane] = s_mb[lane] + n_mb;     // + the cotangent of point 0
  if (lane < 49) grad_cov_in[b * 49 + lane] = s_g[lane] + n_cb;
}

// ---------------------------------------------------------------------------------------
// k_trace_energy_bwd: one lane per sample, behind k_build_bwd on the same stream.  The energy at point k is
// E_in + sum of V cos(phi) over the gaining cavities in front of it (k_trace_reference), so with
// carry_s = sum of energy_bar[k] over k > s -- the cotangent of the energy leaving step s, as in step 4 of
// k_build_bwd -- a gaining cavity at step s receives carry_s dE/dV, carry_s dE/dphase and the incoming energy the
// sum over all points.  Adds into grad_params and grad_energy.
// ---------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(64) void k_trace_energy_bwd(LatticeDev lat, const T* __restrict__ steps,
                                                         const T* __restrict__ energy_bar /* [B][P] */,
                                                         T* __restrict__ grad_params /* [B][E][8] */,
                                                         T* __restrict__ grad_energy /* [B] */) {
  const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (b >= lat.batch) return;
  const int S = lat.n_steps, P = S + 1, E = lat.n_elems;
  const T* pool = static_cast<const T*>(lat.pool);
  T carry = T(0);
  for (int s = S - 1; s >= 0; --s) {
    carry += energy_bar[b * P + s + 1];
    const int desc = (int)steps[(b * S + s) * LYNX_STEP_STRIDE + LYNX_FLAGS_OFFSET];
    if (((desc >> LYNX_DESC_KIND_SHIFT) & 3) == LYNX_STEP_CAVITY && (desc & LYNX_FLAG_CAV_GAIN)) {
      const int first = lat.steps[s].first;
      const lynx_elem el = lat.elems[first];
      const T* p = pool + el.param_offset + b * (int64_t)el.batch_stride;
      const T phi = p[2] * T(LYNX_PI / 180.0);
      T* gp = grad_params + (b * E + first) * (int64_t)kGradParams;
      gp[1] += carry * t_cos(phi);                                   // dE_out/dV
      gp[2] += carry * (-p[1] * t_sin(phi)) * T(LYNX_PI / 180.0);    // dE_out/dphase[deg]
    }
  }
  grad_energy[b] += carry + energy_bar[b * P];
}

// ---------------------------------------------------------------------------------------
// k_trace_trajectories_bwd: grid = B, one wave per sample.  The gradient of a function of the coordinates of K chosen
// particles at every point (what k_trace_trajectories wrote, [B][P][K][7]) is, per particle, the treatment
// k_trace_moments_bwd gives mu -- a single trajectory is differentiable through a cavity's kick, so this sweep has no
// "moments are not closed" case:
//
//   lambda_j = w[S][j]
//   for s = S - 1 .. 0:                     (z = trajectories[s][j], the state that ENTERS step s)
//     gaining cavity: kick_cotangents(z[4], z[5], lambda[4], lambda[5]) -> cc[8], dir4, dir5;  lambda[5] = 0
//     T_bar[s] += lambda (x) z,  coef_bar[s] += cc          (summed over the chosen particles)
//     lambda <- M^T lambda;  lambda[4] += dir4, lambda[5] += dir5;  lambda += w[s][j]
//   grad_chosen_in[j] = lambda
//
// A tile is 64 x kChosenBwdSlots chosen particles: chosen particle j of the tile sits in lane j % 64, slot j / 64 -- the
// layout k_trace_trajectories stored, so a slot's loads of z and of w are one contiguous run per wave.  lambda (7 per
// slot) stays in registers; the step's row is wave-uniform and comes through scalar loads; the row, z and w of step
// s - 1 are fetched while step s is worked on.  Per step a lane forms its 49 + 8 products, summed over its slots, and
// the wave adds them with the trace's halving butterflies, two slabs of 32 = one kGradStride row: afterwards lanes 2 c and
// 2 c + 1 hold the sum of cell c of the slab, the even lane writes the first slab's cell, the odd lane the second's.  K
// beyond one tile: the same wave takes the tiles in order and carries the row sums in float64 (`partial`, [B][S][64]);
// the last tile adds what k_trace_moments_bwd left in tbar (`add_to_tbar`; otherwise tbar is written, not added to) and
// rounds once.  One lane owns every cell it reads and writes, the order is fixed, no atomics: the same call returns the
// same bits, and a particle's lambda depends on nothing but its own z and w -- two rows of a repeated index are equal.
// Arithmetic and sums are float64 for both lattice dtypes (the head of this file); z is read in the lattice's dtype.
// A lane beyond K carries chosen particle K - 1 with lambda = 0 and w = 0: finite work, zeros into every sum.
// ---------------------------------------------------------------------------------------
constexpr int kChosenBwdSlots = 2;

template <typename T>
__global__ __launch_bounds__(64) void k_trace_trajectories_bwd(int S, int64_t K, const T* __restrict__ steps,
                                                               const T* __restrict__ trajectories,
                                                               const double* __restrict__ trajectories_bar,
                                                               T* __restrict__ tbar, double* __restrict__ partial /* null: one tile */,
                                                               int add_to_tbar, T* __restrict__ grad_chosen_in) {
  using A = double;
  constexpr int U = kChosenBwdSlots;
  constexpr int64_t kTile = 64 * U;
  constexpr int kRow = LYNX_COEF_OFFSET + 8;  // what the sweep reads of a step's row: the map and the kick's coefficients
  static_assert(2 * kTraceSlab == kGradStride, "two slabs of the butterfly are one row of tbar");
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x, P = S + 1;
  const int64_t tiles = (K + kTile - 1) / kTile;
  const T* g_steps = steps + b * (int64_t)S * LYNX_STEP_STRIDE;
  const T* g_z = trajectories + b * (int64_t)P * K * 7;
  const double* g_w = trajectories_bar + b * (int64_t)P * K * 7;
  T* g_tbar = tbar + b * (int64_t)S * kGradStride;
  double* g_part = tiles > 1 ? partial + b * (int64_t)S * kGradStride : nullptr;
  const int cell = (lane & 1) ? kTraceSlab + (lane >> 1) : (lane >> 1);

  for (int64_t tile = 0; tile < tiles; ++tile) {
    const bool first = tile == 0, last = tile == tiles - 1;
    bool chosen[U];
    int64_t at[U];  // this slot's particle inside a point's [K][7]
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t j = tile * kTile + lane + 64 * u;
      chosen[u] = j < K;
      at[u] = (chosen[u] ? j : K - 1) * 7;
    }
    A lam[U][7];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int c = 0; c < 7; ++c) {
        const A w = g_w[(int64_t)S * K * 7 + at[u] + c];
        lam[u][c] = chosen[u] ? w : A(0);
      }
    // what step s needs from memory, fetched one step ahead
    T n_z[U][7], n_m[kRow];
    A n_w[U][7];
    int n_desc;
    auto fetch = [&](int s) {
      const T* tab = g_steps + (int64_t)s * LYNX_STEP_STRIDE;  // wave-uniform: scalar loads
      n_desc = (int)uniform_value(tab[LYNX_FLAGS_OFFSET]);
#pragma unroll
      for (int q = 0; q < kRow; ++q) n_m[q] = uniform_value(tab[q]);
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int c = 0; c < 7; ++c) {
          n_z[u][c] = g_z[(int64_t)s * K * 7 + at[u] + c];
          n_w[u][c] = g_w[(int64_t)s * K * 7 + at[u] + c];
        }
    };
    fetch(S - 1);
    for (int s = S - 1; s >= 0; --s) {
      A z[U][7], w[U][7], m[kRow];
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int c = 0; c < 7; ++c) {
          z[u][c] = (A)n_z[u][c];
          w[u][c] = chosen[u] ? n_w[u][c] : A(0);
        }
#pragma unroll
      for (int q = 0; q < kRow; ++q) m[q] = (A)n_m[q];
      const int desc = n_desc;
      if (s > 0) fetch(s - 1);

      const bool kick = ((desc >> LYNX_DESC_KIND_SHIFT) & 3) == LYNX_STEP_CAVITY && (desc & LYNX_FLAG_CAV_GAIN);  // uniform
      A cc[8], dir4[U], dir5[U];
#pragma unroll
      for (int q = 0; q < 8; ++q) cc[q] = A(0);
#pragma unroll
      for (int u = 0; u < U; ++u) dir4[u] = dir5[u] = A(0);
      if (kick) {
        const A* cf = m + LYNX_COEF_OFFSET;
        A sphi, cphi;
        phase_sincos(cf[LYNX_C_PHI], sphi, cphi);
#pragma unroll
        for (int u = 0; u < U; ++u) {
          A kc[8];
          kick_cotangents<A, A>(cf, sphi, cphi, z[u][4], z[u][5], lam[u][4], lam[u][5], kc, dir4[u], dir5[u]);
#pragma unroll
          for (int q = 0; q < 8; ++q) cc[q] += kc[q];
          lam[u][5] = A(0);  // the linear delta was overwritten by the kick
        }
      }
      // cells 0..31 and 32..63 of the row: 49 entries of lambda (x) z, the 8 coefficient cotangents, padding
      A total[2];
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        A v[kTraceSlab];
#pragma unroll
        for (int q = 0; q < kTraceSlab; ++q) {
          const int c = half * kTraceSlab + q;
          if (c < 49) {
            A acc = lam[0][c / 7] * z[0][c % 7];
#pragma unroll
            for (int u = 1; u < U; ++u) acc = fma(lam[u][c / 7], z[u][c % 7], acc);
            v[q] = acc;
          } else if (c < 57) {
            v[q] = cc[c - 49];
          } else {
            v[q] = A(0);
          }
        }
        total[half] = trace_wave_sums<A>(v, lane);
      }
      {
        A sum = (lane & 1) ? total[1] : total[0];
        const int64_t o = (int64_t)s * kGradStride + cell;
        if (!first) sum += g_part[o];
        if (last) {
          if (add_to_tbar) sum += (A)g_tbar[o];
          g_tbar[o] = (T)sum;
        } else {
          g_part[o] = sum;
        }
      }
      // lambda <- M^T lambda, the kick's direct terms, the cotangent of point s
#pragma unroll
      for (int u = 0; u < U; ++u) {
        A o[7];
#pragma unroll
        for (int i = 0; i < 7; ++i) {
          A acc = m[i] * lam[u][0];
#pragma unroll
          for (int k = 1; k < 7; ++k) acc = fma(m[k * 7 + i], lam[u][k], acc);
          o[i] = acc;
        }
        o[4] += dir4[u];
        o[5] += dir5[u];
#pragma unroll
        for (int i = 0; i < 7; ++i) lam[u][i] = o[i] + w[u][i];
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (chosen[u]) {
        T* out = grad_chosen_in + b * K * 7 + at[u];
#pragma unroll
        for (int c = 0; c < 7; ++c) out[c] = (T)lam[u][c];
      }
  }
}

// ---------------------------------------------------------------------------------------
// The reverse pass of a trace WITH LOSSES (lynx_track_particles_along_backward_losses).  The record of point p is taken
// over the particles alive there, and that set changes behind every active aperture -- but the sets are nested and
// locally constant in the parameters, and for a FIXED set of particles the mean and the biased covariance obey the
// recursion above from point 0 on (an aperture step is the identity).  With the apertures at the steps
// a_0 < ... < a_{A-1} and Z_j the incoming particles alive behind the first j of them, the record of point p stands for
// Z_j with j = #{a < p}: Z_j's live points are a_{j-1} + 1 .. a_j (a_{-1} = -1, a_A = S).  So L = sum_j L_j, and L_j is
// the no-loss problem on the moment trace of Z_j with the cotangents zeroed outside its live points.
//
// k_trace_moments_bwd_sets: grid = B * (A + 1), one wave per (sample, set), 49 lanes busy.
//   states      mean and C of set j's incoming particles (lynx_moments_by_loss) taken through the step table from point 0
//               to the set's last live point -- moment_step_wave in float64 whatever the lattice's dtype (the
//               head of this file) -- every state that ENTERS a step parked in `states` [B][A + 1][S][56];
//   cotangents  read from the record cotangents under k_trace_records_to_states' conventions, zero outside the live points;
//   sweep       sweep_products from the last live point down to step 0 (no cavity: refused by the host), T_bar
//               in float64 into the set's own slab `tbar_sets` [A + 1][B][S][64]; rows behind the last live point are 0.
// A set nobody is in (count 0, NaN moments) writes zeros.  k_trace_sum_sets then adds the sets' slabs in set order and
// rounds once into the T_bar k_build_bwd consumes.  One lane owns every cell, fixed order: the same call, the same bits.
// ---------------------------------------------------------------------------------------
constexpr int kMaxLossSets = 16;  // 15 apertures
constexpr int kSetState = 56;     // mu [7] | C [49]

struct TraceLossSets {
  int32_t sets;                // A + 1
  int32_t last[kMaxLossSets];  // last live point of set j: the step of aperture j; S for the last set
};

template <typename T>
__global__ __launch_bounds__(64) void k_trace_moments_bwd_sets(int S, int64_t B, TraceLossSets sets, const T* __restrict__ steps,
                                                               const double* __restrict__ set_records,
                                                               const double* __restrict__ grad_trace,
                                                               double* __restrict__ states, double* __restrict__ tbar_sets) {
  using A = double;
  __shared__ A s_mu[8], s_c[49], s_x[49], s_y[49], s_g[49], s_mb[8], s_m[64];
  const int J = sets.sets;
  const int64_t b = blockIdx.x / J;
  const int set = (int)(blockIdx.x - b * J);
  const int lane = threadIdx.x;
  const int cl = lane < 49 ? lane : 48, l7 = lane < 7 ? lane : 6;
  const int i = cl / 7, j = cl % 7;
  const int L = sets.last[set], lo = set == 0 ? 0 : sets.last[set - 1] + 1;  // live points lo .. L
  const T* g_steps = steps + b * (int64_t)S * LYNX_STEP_STRIDE;
  const double* rec = set_records + (b * J + set) * (int64_t)LYNX_MOMENT_STRIDE;
  const double* g = grad_trace + b * (int64_t)(S + 1) * LYNX_MOMENT_STRIDE;
  double* st = states + (b * J + set) * (int64_t)S * kSetState;
  double* out = tbar_sets + ((int64_t)set * B + b) * (int64_t)S * kGradStride;
  const bool empty = rec[35] == 0.0;  // uniform
  for (int s = empty ? 0 : L; s < S; ++s) out[(int64_t)s * kGradStride + lane] = 0.0;
  if (empty) return;
  // this lane's entry in a record's triangle (k_trace_records_to_states)
  const bool inner = i < 6 && j < 6;
  const int r = i < j ? i : j, q = i < j ? j : i;
  const int tri = inner ? 7 + r * 6 - (r * (r - 1)) / 2 + (q - r) : 7;
  const A weight = !inner ? 0.0 : (i == j ? 1.0 : 0.5);

  // forward: the state entering step s parked at st[s]
  if (lane < 7) s_mu[lane] = lane < 6 ? rec[lane] : 1.0;
  if (lane < 49) s_c[lane] = inner ? rec[tri] : 0.0;
  __syncthreads();
  for (int s = 0; s < L; ++s) {
    if (lane < 7) st[(int64_t)s * kSetState + lane] = s_mu[lane];
    if (lane < 49) st[(int64_t)s * kSetState + 7 + lane] = s_c[lane];
    s_m[lane] = (A)g_steps[(int64_t)s * LYNX_STEP_STRIDE + lane];
    __syncthreads();
    moment_step_wave<A>(s_m, s_mu, s_c, s_x, lane, i, j, false);  // (no cavity: refused by the host)
  }
  __threadfence_block();
  __syncthreads();

  // reverse, with k_trace_moments_bwd's prefetching: the cotangent of point p counts for lo <= p <= L (point 0's reaches no parameter)
  if (lane < 7) s_mb[lane] = A(0);
  if (lane < 49) s_g[lane] = A(0);
  A n_mu = A(0), n_c = A(0), n_m = A(0), n_mb = A(0), n_cb = A(0);
  if (L > 0) {
    n_mb = L >= lo ? g[(int64_t)L * LYNX_MOMENT_STRIDE + l7] : A(0);
    n_cb = L >= lo ? weight * g[(int64_t)L * LYNX_MOMENT_STRIDE + tri] : A(0);
    n_mu = st[(int64_t)(L - 1) * kSetState + l7];
    n_c = st[(int64_t)(L - 1) * kSetState + 7 + cl];
    n_m = (A)g_steps[(int64_t)(L - 1) * LYNX_STEP_STRIDE + lane];
  }
  __syncthreads();
  for (int s = L - 1; s >= 0; --s) {
    if (lane < 7) {
      s_mb[lane] += n_mb;  // cotangent of point s + 1
      s_mu[lane] = n_mu;   // state at point s
    }
    if (lane < 49) {
      s_g[lane] += n_cb;
      s_c[lane] = n_c;
    }
    s_m[lane] = n_m;
    if (s > 0) {
      const bool counts = s >= lo;  // uniform
      n_mb = counts ? g[(int64_t)s * LYNX_MOMENT_STRIDE + l7] : A(0);
      n_cb = counts ? weight * g[(int64_t)s * LYNX_MOMENT_STRIDE + tri] : A(0);
      n_mu = st[(int64_t)(s - 1) * kSetState + l7];
      n_c = st[(int64_t)(s - 1) * kSetState + 7 + cl];
      n_m = (A)g_steps[(int64_t)(s - 1) * LYNX_STEP_STRIDE + lane];
    }
    __syncthreads();
    A tb, cb, mbn;
    sweep_products<A>(s_m, s_mu, s_c, s_g, s_mb, s_x, s_y, lane, i, j, tb, cb, mbn);
    out[(int64_t)s * kGradStride + lane] = lane < 49 ? tb : A(0);
    __syncthreads();
    if (lane < 49) s_g[lane] = cb;
    if (lane < 7) s_mb[lane] = mbn;
    __syncthreads();
  }
}

// grid = ceil(cells / 256): cell c of T_bar [B][S][64] is the sum over the sets of cell c of their slabs, in set order
template <typename T>
__global__ __launch_bounds__(256) void k_trace_sum_sets(const double* __restrict__ tbar_sets, int sets, int64_t cells,
                                                        T* __restrict__ tbar) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= cells) return;
  double v = 0.0;
  for (int j = 0; j < sets; ++j) v += tbar_sets[(int64_t)j * cells + c];
  tbar[c] = (T)v;
}

}  // namespace lynx

// gfx950 kernels of the beam trace: the moments of the beam at the entrance and behind EVERY element of a
// lattice from one pass over the particles (lynx_track_particles_along), and the ParameterBeam's counterpart
// (lynx_track_moments_along).  Included only by lynx_hip.hip, behind lynx_device.hpp.
//
// What the reference does for this is the loop of `Segment.plot_twiss` (segment.py: `element.track(beam)` element by
// element, `beta_x`, `beta_y` of every intermediate beam): 2 E passes over the particle array.  Here:
//
//   table      [B][E][64]   every element a step of its own (the existing builders; LYNX_STEP_FLAG_RAW)
//   k_trace_reference       one wave per sample takes 64 CANDIDATES (particle 0 and 63 more at equal strides) through the
//                           E steps and the apertures of the call (none: no walk, every finite candidate counts),
//                           takes the component-wise median -- at the entrance -- of those that stay alive and finite
//                           to the end (none does: of those that do longest) through the steps and writes its
//                           coordinates at every point, [B][P][8], next to
//                           the beam energy there, [B][P].  That trajectory is the reference point the sums of every
//                           point are taken about: it moves with the centroid (correctors, misaligned quadrupoles, a
//                           cavity's delta), so float32 products do not cancel; it lies inside the beam at every point
//                           whichever particle is stored first and whatever becomes of the lost ones; it is the same
//                           for every wave of a sample, so the records add up as they are.
//   k_trace_particles       a wave loads a tile of 64 U particles ONCE, keeps them in registers and takes them through
//                           the E steps; at every point each lane forms the 28 shifted sums of its U particles
//                           (6 first moments, the 7th column, 21 products), the wave folds them with a transposing
//                           butterfly (32 exchanges for all 28 sums, not 6 x 28) and adds the result into ITS OWN
//                           float64 slab [P][32] in memory -- the same lane reads and writes the same cell, tile after
//                           tile: no atomics, one fixed order.
//   k_trace_finalize        adds the waves' slabs of a (sample, point) in a fixed order and writes the moment record
//                           [B][P][36] (layout of LYNX_MOMENT_STRIDE, slot 34 = 1).
//
// The three particle kernels are one wave body (trace_wave) instantiated three times -- the flags decide the register
// pressure -- and a lattice with active apertures or screens comes with ONE step plan (TraceLosses.plan): a code per
// step that says "nothing", "aperture k" or "screen k", read by one hook behind every point (trace_step_hook).
//
// With particle losses (lynx_track_particles_along_losses; k_trace_particles_losses) an active aperture is an identity
// step that clears the `live` bit of the particles outside it: nothing is compacted, a lost particle stays in its lane
// and is kept out of every later sum by a select, and the number of particles a record stands for is the point's own
// sum of the 7th coordinate (slot 6 of the slab row) instead of N (k_trace_finalize with a negative count).
//
// The reverse pass of such a trace wants the moments of the INCOMING beam over every nested survivor set
// (lynx_moments_by_loss; k_moments_by_loss): the same wave body's pieces with identity steps, the sets for points.
//
// With screens (lynx_track_particles_along_screens; k_trace_particles_screens) an active screen is an identity step too:
// the particles alive where it stands are binned by numpy's rule on the screen's own edge arrays (bin_of's result, from
// an arithmetic guess corrected against the neighbouring edges) and counted into the screen's image with integer
// atomics -- there, because the particles of an interior point exist in registers only.
//
// With trajectories (lynx_track_particles_along_trajectories; k_trace_trajectories) a second, small kernel behind the
// particle kernel of the same call takes K CHOSEN particles through the same table and the same plan and writes their
// coordinates at every point, [B][P][K][7] -- the data of the reference's plot_reference_particle_traces (segment.py:
// `xs[particle]`, `ys[particle]` behind every split element), which the moment records do not hold.  The particle
// kernels above do not know about it.
#pragma once

#include "lynx_device.hpp"

namespace lynx {

constexpr int kTraceSlab = 32;  // float64 cells per (wave, point): 28 sums, padded to a power of two for the butterfly
constexpr int kTraceRef = 8;    // scalars per (sample, point) of the reference trajectory (6 used)

struct TraceArgs {
  int64_t n_particles;
  int64_t in_stride;      // scalars between the samples of p_in: N * 7, or 0 for one shared incoming beam
  int32_t waves;          // waves per sample (a multiple of 4: whole workgroups)
  int32_t tiles_per_wave;
  int32_t store;          // 1: write p_out
  int32_t points;         // P = E + 1
};

// The step plan of a trace with apertures and / or screens, and its apertures.  `plan`: [S] step codes, then [K][4] per
// screen (K may be 0).  A step's code is -1, (ordinal of the aperture << 2) | (elliptical << 1) for an active aperture,
// (ordinal of the screen << 2) | 1 for an active screen; a screen's row is nx, ny, the first scalar of its edges in
// TraceScreens.edges (x edges, nx + 1 of them, then y edges), the first cell of its image in a sample's row of
// TraceScreens.images.  `limits` [B or 1][A][2]: x_max, y_max in the lattice's dtype (not read without apertures).
struct TraceLosses {
  const int64_t* plan;
  const void* limits;
  int64_t limit_stride;  // scalars between the samples of `limits`: 2 A, or 0 for limits the batch shares
  int32_t* lost_at;      // [B][N], -1 everywhere before the launch: a particle's cell is written when (and if) an aperture
                         // removes it, with the aperture's ordinal (keeping the ordinals in registers until the end of
                         // the tile costs the float32 kernel its third wave per SIMD); or null
};

// The screens of a trace (which steps they are, and their rows: TraceLosses.plan).
struct TraceScreens {
  const void* edges;          // lattice dtype
  const void* misalignment;   // [B or 1][K][2], lattice dtype
  int64_t misalignment_stride;  // scalars between the samples of `misalignment`: 2 K, or 0
  int32_t* images;            // [B][cells] int32, zero before the launch
  int64_t cells;              // sum over the screens of ny nx
};

// ---------------------------------------------------------------------------------------
// The reference point of a sample's sums.  64 CANDIDATES, one per lane: particle 0 and 63 more at equal strides over the
// sample (lane l: particle floor(l N / 64); N < 64: some particles more than once).  Every candidate has a score, the
// number of points (of sets, in k_moments_by_loss) it is a finite, living member of; the candidates of the highest score
// are the ones that stay in the beam longest, and the reference point is their component-wise median (the lower one of an
// even number): no particle of the beam as a rule, and none is needed -- k_trace_finalize only adds the point back.  A
// candidate that is lost, far out or not finite does not move the median of the others; the guarantee ends where fewer
// than half of the best candidates lie inside the set a record is about.  No candidate finite at the entrance: the origin.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t trace_candidate(int lane, int64_t n) { return (n / 64) * lane + (n % 64) * lane / 64; }

template <typename T>
__device__ __forceinline__ bool trace_finite(const T (&z)[7]) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 6; ++k) ok = ok && __builtin_isfinite(z[k]);
  return ok;
}

// `v` of the 64 lanes in ascending order, lane by lane: a bitonic network, 21 exchanges (no NaN among them).
template <typename T>
__device__ __forceinline__ T trace_wave_sorted(T v, int lane) {
#pragma unroll
  for (int k = 2; k <= 64; k <<= 1)
#pragma unroll
    for (int j = k >> 1; j >= 1; j >>= 1) {
      const T other = __shfl_xor(v, j, 64);
      const bool smaller = ((lane & j) == 0) == ((lane & k) == 0);  // this lane keeps the smaller one of the pair
      v = smaller ? (other < v ? other : v) : (other > v ? other : v);
    }
  return v;
}

template <typename T>
__device__ __forceinline__ void trace_reference_median(const T (&z)[7], int score, int lane, T (&c)[6]) {
  int best = score;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) best = max(best, __shfl_xor(best, m, 64));
  const bool mine = best > 0 && score == best;
  const int members = __popcll(__ballot(mine));
#pragma unroll
  for (int k = 0; k < 6; ++k) {  // the others sort behind the set: +inf
    const T sorted = trace_wave_sorted<T>(mine ? z[k] : T(__builtin_huge_valf()), lane);
    c[k] = members > 0 ? __shfl(sorted, (members - 1) / 2, 64) : T(0);
  }
}

// The rows of the steps s0 .. s0 + kTraceRefChunk - 1 of a sample (as many as there are) into LDS, by one wave: every
// lane's loads are in flight at once, so a chunk costs one memory latency -- read from memory step by step, the walk
// below paid one per step (1.2 us each: 0.15 ms for 128 elements).
constexpr int kTraceRefChunk = 32;

template <typename T>
__device__ __forceinline__ void trace_stage_steps(const T* __restrict__ sample_steps, int S, int s0, T* __restrict__ rows, int lane) {
  const int count = min(kTraceRefChunk, S - s0) * LYNX_STEP_STRIDE;
  const T* src = sample_steps + (int64_t)s0 * LYNX_STEP_STRIDE;
  __syncthreads();  // (one wave: what it still reads of the chunk before)
#pragma unroll
  for (int q = 0; q < kTraceRefChunk; ++q) {
    const int i = q * 64 + lane;
    if (i < count) rows[i] = src[i];
  }
  __syncthreads();
}

// ---------------------------------------------------------------------------------------
// k_trace_reference: reference trajectory and energies, one wave per sample.  With apertures (`plan`, `limits_all`:
// TraceLosses' of the call) the lanes take the 64 candidates through the S steps and the apertures -- a candidate's score
// is the number of points it reaches alive and finite --; without them (null) nobody is lost, and the candidates finite
// at the entrance are the best.  The median of the best AT THE ENTRANCE is taken through the steps, and its coordinates
// at every point are the reference points, [B][P][8].  Both walks read the steps' rows from LDS, kTraceRefChunk of them
// staged at a time (trace_stage_steps).
// Energy behind an active cavity: E + V cos(phi), the expression of energy_before_step (cavity.py:130).
// ---------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(64) void k_trace_reference(LatticeDev lat, const T* __restrict__ steps,
                                                        const T* __restrict__ energy_in, const T* __restrict__ p_in,
                                                        int64_t in_stride, int64_t n_particles,
                                                        const int64_t* __restrict__ plan, const T* __restrict__ limits_all,
                                                        int64_t limit_stride, T* __restrict__ ref_out,
                                                        T* __restrict__ energy_trace) {
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x;
  const int S = lat.n_steps, P = S + 1;
  const T* pool = static_cast<const T*>(lat.pool);
  const T* sample_steps = steps + b * (int64_t)S * LYNX_STEP_STRIDE;
  const T* limits = (plan && limits_all) ? limits_all + b * limit_stride : nullptr;
  T first[7], z[7];
  load_particle(p_in + b * in_stride + trace_candidate(lane, n_particles) * 7, first);
#pragma unroll
  for (int k = 0; k < 7; ++k) z[k] = first[k];
  __shared__ T s_rows[kTraceRefChunk * LYNX_STEP_STRIDE];
  __shared__ int s_plan[kTraceRefChunk];
  // without apertures nobody is lost, and a candidate is as good as it is at the entrance: no walk
  int score = trace_finite<T>(first) ? 1 : 0;
  bool alive = true;
  for (int s = 0; limits && s <= S; ++s) {
    alive = alive && trace_finite<T>(z);
    if (alive) score = s + 1;
    if (s == S) break;
    if (s % kTraceRefChunk == 0) {  // (the chunk's codes of the plan with its rows)
      if (lane < min(kTraceRefChunk, S - s)) s_plan[lane] = (int)plan[s + lane];
      trace_stage_steps<T>(sample_steps, S, s, s_rows, lane);
    }
    const int code = __builtin_amdgcn_readfirstlane(s_plan[s % kTraceRefChunk]);
    if (code >= 0 && !(code & 1))  // an active aperture (TraceLosses.plan)
      alive = alive && aperture_survives<T>(z[0], z[2], limits[(code >> 2) * 2], limits[(code >> 2) * 2 + 1], (code >> 1) & 1);
    const T* M = s_rows + (s % kTraceRefChunk) * LYNX_STEP_STRIDE;
    const int desc = (int)M[LYNX_FLAGS_OFFSET];
    apply_step<T>(M, (desc >> LYNX_DESC_KIND_SHIFT) & 3, desc & 0xffff, z);
  }
  T c[6];
  trace_reference_median<T>(first, score, lane, c);
#pragma unroll
  for (int k = 0; k < 6; ++k) z[k] = c[k];
  z[6] = T(1);
  T e = energy_in[b];
  for (int s = 0; s <= S; ++s) {  // (every lane the same point; lane 0 writes)
    if (lane == 0) {
      T* r = ref_out + (b * P + s) * kTraceRef;
#pragma unroll
      for (int k = 0; k < 7; ++k) r[k] = z[k];
      r[7] = T(0);
      energy_trace[b * P + s] = e;
    }
    if (s == S) break;
    // (a lattice of one chunk is still there from the candidates' walk)
    if (s % kTraceRefChunk == 0 && (S > kTraceRefChunk || !limits)) trace_stage_steps<T>(sample_steps, S, s, s_rows, lane);
    const T* M = s_rows + (s % kTraceRefChunk) * LYNX_STEP_STRIDE;
    const int desc = (int)M[LYNX_FLAGS_OFFSET];
    const int skind = (desc >> LYNX_DESC_KIND_SHIFT) & 3, sflags = desc & 0xffff;
    apply_step<T>(M, skind, sflags, z);
    if (skind == LYNX_STEP_CAVITY && (sflags & LYNX_FLAG_CAV_GAIN)) {
      const lynx_elem el = lat.elems[lat.steps[s].first];
      const T* p = pool + el.param_offset + b * (int64_t)el.batch_stride;
      e = e + p[1] * t_cos(p[2] * T(LYNX_PI / 180.0));
    }
  }
}

// k_trace_energies: the energies alone (a ParameterBeam's trace), one lane per sample.
template <typename T>
__global__ __launch_bounds__(64) void k_trace_energies(LatticeDev lat, const T* __restrict__ steps,
                                                       const T* __restrict__ energy_in, T* __restrict__ energy_trace) {
  const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (b >= lat.batch) return;
  const int S = lat.n_steps, P = S + 1;
  const T* pool = static_cast<const T*>(lat.pool);
  T e = energy_in[b];
  for (int s = 0; s <= S; ++s) {
    energy_trace[b * P + s] = e;
    if (s == S) break;
    const int desc = (int)steps[(b * S + s) * LYNX_STEP_STRIDE + LYNX_FLAGS_OFFSET];
    if (((desc >> LYNX_DESC_KIND_SHIFT) & 3) == LYNX_STEP_CAVITY && (desc & LYNX_FLAG_CAV_GAIN)) {
      const lynx_elem el = lat.elems[lat.steps[s].first];
      const T* p = pool + el.param_offset + b * (int64_t)el.batch_stride;
      e = e + p[1] * t_cos(p[2] * T(LYNX_PI / 180.0));
    }
  }
}

// ---------------------------------------------------------------------------------------
// The transposing butterfly: every lane holds 32 values; afterwards v[0] of lane l is the sum over all 64 lanes of
// value (l >> 1).  Level by level a lane keeps one half of its values and hands the other half to the lane whose
// index differs in one bit: 16 + 8 + 4 + 2 + 1 exchanges, then one more between neighbours.
// ---------------------------------------------------------------------------------------
// The two widest levels (partner 32 and 16 lanes away) as gfx950's lane swaps: v_permlane32_swap exchanges the upper
// half of its first operand with the lower half of its second, v_permlane16_swap the odd rows of 16 lanes of the first
// with the even rows of the second -- afterwards one register holds, in every lane, this lane's kept value and the
// other the value it was handed: one swap and one add per pair, no select, nothing through the LDS crossbar.
template <int HALF>
__device__ __forceinline__ void trace_lane_swap(unsigned& a, unsigned& b) {
  static_assert(HALF == 16 || HALF == 8, "partner 32 or 16 lanes away");
  if constexpr (HALF == 16) {
    const auto r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
    a = r[0];
    b = r[1];
  } else {
    const auto r = __builtin_amdgcn_permlane16_swap(a, b, false, false);
    a = r[0];
    b = r[1];
  }
}
template <int HALF>
__device__ __forceinline__ float trace_swap_add(float lo, float hi) {
  unsigned a = __float_as_uint(lo), b = __float_as_uint(hi);
  trace_lane_swap<HALF>(a, b);
  return __uint_as_float(a) + __uint_as_float(b);
}
template <int HALF>
__device__ __forceinline__ double trace_swap_add(double lo, double hi) {
  const unsigned long long x = (unsigned long long)__double_as_longlong(lo), y = (unsigned long long)__double_as_longlong(hi);
  unsigned a0 = (unsigned)(x & 0xffffffffull), a1 = (unsigned)(x >> 32), b0 = (unsigned)(y & 0xffffffffull), b1 = (unsigned)(y >> 32);
  trace_lane_swap<HALF>(a0, b0);
  trace_lane_swap<HALF>(a1, b1);
  return __longlong_as_double((long long)(((unsigned long long)a1 << 32) | a0)) +
         __longlong_as_double((long long)(((unsigned long long)b1 << 32) | b0));
}

template <typename R, int HALF>
__device__ __forceinline__ void trace_fold(R (&v)[kTraceSlab], int lane) {
  if constexpr (HALF >= 8) {
#pragma unroll
    for (int i = 0; i < HALF; ++i) v[i] = trace_swap_add<HALF>(v[i], v[i + HALF]);
    return;
  }
  const bool up = (lane & (HALF * 2)) != 0;
#pragma unroll
  for (int i = 0; i < HALF; ++i) {
    const R keep = up ? v[i + HALF] : v[i];
    const R send = up ? v[i] : v[i + HALF];
    v[i] = keep + __shfl_xor(send, HALF * 2, 64);
  }
}
template <typename R>
__device__ __forceinline__ R trace_wave_sums(R (&v)[kTraceSlab], int lane) {
  trace_fold<R, 16>(v, lane);
  trace_fold<R, 8>(v, lane);
  trace_fold<R, 4>(v, lane);
  trace_fold<R, 2>(v, lane);
  trace_fold<R, 1>(v, lane);
  return v[0] + __shfl_xor(v[0], 1, 64);
}

__device__ __forceinline__ double vfma(double a, double b, double c) { return fma(a, b, c); }

// products of the shifted coordinates, the 21 of the upper triangle, spelled out by recursion (see LaneSums)
template <typename V, int K>
__device__ __forceinline__ void trace_products(const V (&e)[6], V (&acc)[28]) {
  if constexpr (K < 21) {
    constexpr int r = MomentSet<true>::tri_row(K), c = MomentSet<true>::tri_col(K);
    acc[7 + K] = vfma(e[r], e[c], acc[7 + K]);
    trace_products<V, K + 1>(e, acc);
  }
}
// This wave's sums at one point: into cell (lane >> 1) of the point's slab row.
template <typename R>
__device__ __forceinline__ void trace_deposit(R (&v)[kTraceSlab], int lane, bool first, double* __restrict__ row) {
  const R total = trace_wave_sums<R>(v, lane);
  if ((lane & 1) == 0) {
    double* cell = row + (lane >> 1);
    const double before = first ? 0.0 : *cell;
    *cell = before + (double)total;
  }
}

// float32: two particles per lane as packed pairs (apply_step_pair: the same operations in the same order per
// component as apply_step<float>), the sums of a pair in packed registers as well -- v_pk_fma_f32 / v_pk_add_f32 for
// the map AND the 27 accumulations; the two halves are added when the lane's values go into the butterfly.
template <int U, bool MASKED>
__device__ __forceinline__ void trace_point(const lynx_f32x2 (&zp)[U / 2][7], const float* __restrict__ ref,
                                            const bool (&live)[U], int lane, bool first, double* __restrict__ row) {
  lynx_f32x2 acc[28];
#pragma unroll
  for (int k = 0; k < 28; ++k) acc[k] = lynx_f32x2{0.f, 0.f};
  float c[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) c[k] = uniform_value(ref[k]);
#pragma unroll
  for (int h = 0; h < U / 2; ++h) {
    lynx_f32x2 e[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      e[k] = zp[h][k] - lynx_f32x2{c[k], c[k]};
      if (MASKED) {
        e[k].x = live[2 * h] ? e[k].x : 0.f;
        e[k].y = live[2 * h + 1] ? e[k].y : 0.f;
      }
      acc[k] += e[k];
    }
    lynx_f32x2 one = zp[h][6];
    if (MASKED) {
      one.x = live[2 * h] ? one.x : 0.f;
      one.y = live[2 * h + 1] ? one.y : 0.f;
    }
    acc[6] += one;
    trace_products<lynx_f32x2, 0>(e, acc);
  }
  float v[kTraceSlab];
#pragma unroll
  for (int k = 0; k < 28; ++k) v[k] = acc[k].x + acc[k].y;
#pragma unroll
  for (int k = 28; k < kTraceSlab; ++k) v[k] = 0.f;
  trace_deposit<float>(v, lane, first, row);
}

// float64: one particle at a time, everything in float64
template <int U, bool MASKED>
__device__ __forceinline__ void trace_point(const double (&z)[U][7], const double* __restrict__ ref,
                                            const bool (&live)[U], int lane, bool first, double* __restrict__ row) {
  double acc[28];
#pragma unroll
  for (int k = 0; k < 28; ++k) acc[k] = 0.0;
  double c[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) c[k] = ref[k];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    double e[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      e[k] = z[u][k] - c[k];
      if (MASKED) e[k] = live[u] ? e[k] : 0.0;
      acc[k] += e[k];
    }
    acc[6] += (MASKED && !live[u]) ? 0.0 : z[u][6];
    trace_products<double, 0>(e, acc);
  }
  double v[kTraceSlab];
#pragma unroll
  for (int k = 0; k < 28; ++k) v[k] = acc[k];
#pragma unroll
  for (int k = 28; k < kTraceSlab; ++k) v[k] = 0.0;
  trace_deposit<double>(v, lane, first, row);
}

// Step s of a trace with losses, after point s has been deposited, if the step is the aperture `code` >> 1 (elliptical:
// `code` & 1; wave-uniform): the particles whose coordinates ENTERING it lie outside are dead from the next point on.
// The comparison is k_aperture_mask's own (aperture_survives<T>, aperture.py:78-86).
template <typename T, int U, typename X>
__device__ __forceinline__ void trace_aperture_coded(int code /* uniform, >= 0 */, const T* __restrict__ limits /* of this sample */,
                                                     X&& xy, bool (&live)[U], int32_t* __restrict__ tile_lost_at /* uniform */, int lane) {
  const int ordinal = code >> 1;
  const T xm = uniform_value(limits[ordinal * 2]), ym = uniform_value(limits[ordinal * 2 + 1]);
#pragma unroll
  for (int u = 0; u < U; ++u) {
    T x, y;
    xy(u, x, y);
    const bool out = live[u] && !aperture_survives<T>(x, y, xm, ym, code & 1);
    if (out && tile_lost_at) tile_lost_at[lane + 64 * u] = ordinal;  // (once: the particle is dead from here on)
    live[u] = live[u] && !out;
  }
}

// The bin of v among n bins with the edges `edges` [n + 1], by numpy.histogramdd's rule: the number of edges <= v, minus
// one; the last edge belongs to the last bin; -1 outside (and for NaN).  bin_of's result without its bisection: the
// edges of a screen are evenly spaced, so (v - first edge) * bins / extent is the bin or one of its neighbours, and the
// comparisons with the very edge values decide -- two loads per axis where the guess holds, any number where it does not.
template <typename T>
__device__ __forceinline__ int screen_bin(const T* __restrict__ edges, int n, T first, T last, T per_unit, T v) {
  if (!(v >= first) || !(v <= last)) return -1;
  int i = (int)((v - first) * per_unit);
  i = min(max(i, 0), n - 1);
  while (i > 0 && v < edges[i]) --i;
  while (i < n - 1 && v >= edges[i + 1]) ++i;
  return i;
}

// Step s of a trace with screens, after point s has been deposited, if the step is screen `ordinal` (wave-uniform): the
// particles alive ENTERING it are counted into its image, flipud(histogramdd((x - misalignment_x, y)).T) of
// screen.py:196-213 (Screen._observe takes the y misalignment off x', which no image sees).  A dead particle is left out
// because it is dead, whatever its coordinates have become.
template <typename T, int U, typename X>
__device__ __forceinline__ void trace_screen(const TraceScreens& scr, const int64_t* __restrict__ rows /* of the plan */, int ordinal,
                                             int64_t b, X&& xy, const bool (&live)[U]) {
  const int64_t* row = rows + 4 * (int64_t)ordinal;
  const int nx = __builtin_amdgcn_readfirstlane((int)row[0]), ny = __builtin_amdgcn_readfirstlane((int)row[1]);
  const T* xe = static_cast<const T*>(scr.edges) + row[2];
  const T* ye = xe + nx + 1;
  int32_t* img = scr.images + b * scr.cells + row[3];
  const T shift = uniform_value(static_cast<const T*>(scr.misalignment)[b * scr.misalignment_stride + 2 * ordinal]);
  const T x_first = uniform_value(xe[0]), x_last = uniform_value(xe[nx]), y_first = uniform_value(ye[0]), y_last = uniform_value(ye[ny]);
  const T x_per_unit = T(nx) / (x_last - x_first), y_per_unit = T(ny) / (y_last - y_first);
  T px[U], py[U];
#pragma unroll
  for (int u = 0; u < U; ++u) xy(u, px[u], py[u]);
  // one particle at a time, picked by a uniform index: unrolled U times, the searches of all U particles were live
  // at once and took the float32 kernel its third wave per SIMD
#pragma nounroll
  for (int u = 0; u < U; ++u) {
    T x = px[0], y = py[0];
    bool alive = live[0];
#pragma unroll
    for (int q = 1; q < U; ++q)
      if (u == q) x = px[q], y = py[q], alive = live[q];
    if (!alive) continue;
    const int ix = screen_bin<T>(xe, nx, x_first, x_last, x_per_unit, x - shift);
    const int iy = screen_bin<T>(ye, ny, y_first, y_last, y_per_unit, y);
    if (ix >= 0 && iy >= 0) atomicAdd(img + (int64_t)(ny - 1 - iy) * nx + ix, 1);  // (no return value: one global_atomic_add)
  }
}

// Step s of a trace with apertures and / or screens, after point s has been deposited: one code of the plan says what
// the step is (wave-uniform: a scalar load).
template <typename T, int U, bool SCREENS, typename X>
__device__ __forceinline__ void trace_step_hook(const TraceLosses& loss, const TraceScreens& scr, const T* __restrict__ limits /* of this sample */,
                                                int S, int s, int64_t b, X&& xy, bool (&live)[U],
                                                int32_t* __restrict__ tile_lost_at /* uniform */, int lane) {
  const int code = __builtin_amdgcn_readfirstlane((int)loss.plan[s]);
  if (code < 0) return;
  if constexpr (SCREENS)
    if (code & 1) return trace_screen<T, U>(scr, loss.plan + S, code >> 2, b, xy, live);
  trace_aperture_coded<T, U>(code >> 1, limits, xy, live, tile_lost_at, lane);
}

// one tile of a wave through the whole lattice
template <typename T, int U, bool MASKED, bool LOSSES, bool SCREENS>
__device__ __forceinline__ void trace_tile(const TraceArgs& a, int S, const T* __restrict__ steps /* of this sample */,
                                           const T* __restrict__ ref /* of this sample */, const T* __restrict__ src,
                                           T* __restrict__ dst, int64_t base, int lane, bool first,
                                           double* __restrict__ slab /* of this wave */, const TraceLosses& loss,
                                           const T* __restrict__ limits, int32_t* __restrict__ lost_at,
                                           const TraceScreens& scr, int64_t b) {
  static_assert(MASKED || !LOSSES, "a trace with losses always takes the masked path");
  static_assert(LOSSES || !SCREENS, "a trace with screens takes the path of the losses (its apertures may be none)");
  bool live[U];
  T z[U][7];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int64_t i = base + lane + 64 * u;
    live[u] = !MASKED || i < a.n_particles;
    // (a lane beyond the end of the sample carries the sample's last particle: finite work, no part in any sum)
    load_particle(src + (live[u] ? i : a.n_particles - 1) * 7, z[u]);
  }
  if constexpr (sizeof(T) == 4) {
    lynx_f32x2 zp[U / 2][7];
#pragma unroll
    for (int u = 0; u < U; u += 2)
#pragma unroll
      for (int c = 0; c < 7; ++c) {
        zp[u / 2][c].x = z[u][c];
        zp[u / 2][c].y = z[u + 1][c];
      }
    for (int s = 0; s <= S; ++s) {
      trace_point<U, MASKED>(zp, ref + s * kTraceRef, live, lane, first, slab + (int64_t)s * kTraceSlab);
      if (s == S) break;
      if constexpr (LOSSES)
        trace_step_hook<T, U, SCREENS>(loss, scr, limits, S, s, b, [&](int u, T& x, T& y) {
          x = (u & 1) ? zp[u / 2][0].y : zp[u / 2][0].x;
          y = (u & 1) ? zp[u / 2][2].y : zp[u / 2][2].x;
        }, live, lost_at ? lost_at + base : nullptr, lane);
      const T* tab = steps + s * LYNX_STEP_STRIDE;  // global, wave-uniform: scalar loads
      const int desc = (int)uniform_value(tab[LYNX_FLAGS_OFFSET]);
      const int skind = (desc >> LYNX_DESC_KIND_SHIFT) & 3, sflags = desc & 0xffff;
      T m[LYNX_STEP_SCALARS];
#pragma unroll
      for (int q = 0; q < LYNX_STEP_SCALARS; ++q) m[q] = uniform_value(tab[q]);
      // apply_step_pair's operations, with the 7x7 of EVERY pair in front of the kicks: the 49 map entries are dead
      // by the time the cosine is called (as one call per pair they were parked in VGPR lanes around each of them)
      lynx_f32x2 o[U / 2][7];
#pragma unroll
      for (int h = 0; h < U / 2; ++h)
#pragma unroll
        for (int i = 0; i < 7; ++i) {
          lynx_f32x2 acc = zp[h][0] * m[i * 7 + 0];
#pragma unroll
          for (int j = 1; j < 7; ++j) acc = pk_fma(zp[h][j], m[i * 7 + j], acc);
          o[h][i] = acc;
        }
      if (skind == LYNX_STEP_CAVITY && (sflags & LYNX_FLAG_CAV_GAIN)) {  // uniform
        const float* coef = m + LYNX_COEF_OFFSET;
#pragma unroll
        for (int h = 0; h < U / 2; ++h) {
          const lynx_f32x2 dcos = cos_difference(-1.0f * zp[h][4] * coef[LYNX_C_BK], coef[LYNX_C_PHI],
                                                 coef[LYNX_SINPHI_OFFSET - LYNX_COEF_OFFSET], coef[LYNX_C_COSPHI]);
          kick_outputs<lynx_f32x2>(coef, zp[h][4], zp[h][5], dcos, o[h][4], o[h][5]);
        }
      }
#pragma unroll
      for (int h = 0; h < U / 2; ++h)
#pragma unroll
        for (int i = 0; i < 7; ++i) zp[h][i] = o[h][i];
    }
#pragma unroll
    for (int u = 0; u < U; u += 2)
#pragma unroll
      for (int c = 0; c < 7; ++c) {
        z[u][c] = zp[u / 2][c].x;
        z[u + 1][c] = zp[u / 2][c].y;
      }
  } else {
    for (int s = 0; s <= S; ++s) {
      trace_point<U, MASKED>(z, ref + s * kTraceRef, live, lane, first, slab + (int64_t)s * kTraceSlab);
      if (s == S) break;
      if constexpr (LOSSES)
        trace_step_hook<T, U, SCREENS>(loss, scr, limits, S, s, b, [&](int u, T& x, T& y) {
          x = z[u][0];
          y = z[u][2];
        }, live, lost_at ? lost_at + base : nullptr, lane);
      const T* tab = steps + s * LYNX_STEP_STRIDE;
      const int desc = (int)tab[LYNX_FLAGS_OFFSET];
      const int skind = (desc >> LYNX_DESC_KIND_SHIFT) & 3, sflags = desc & 0xffff;
#pragma unroll
      for (int u = 0; u < U; ++u) apply_step<T>(tab, skind, sflags, z[u]);
    }
  }
  if constexpr (LOSSES) {
    // (a lost particle is stored as far as it was propagated; its `lost_at` -- written where it was lost -- says so)
    if (a.store) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t i = base + lane + 64 * u;
        if (i < a.n_particles) store_particle(dst + i * 7, z[u]);
      }
    }
  } else if (a.store) {
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (live[u]) store_particle(dst + (base + lane + 64 * u) * 7, z[u]);
  }
}

// ---------------------------------------------------------------------------------------
// The particle kernels: grid.x = B * waves / 4, 256 threads; wave w of a sample owns the particles
// [w * tiles_per_wave * 64 U, (w + 1) * tiles_per_wave * 64 U).  No LDS, no barrier.  A wave whose range lies
// beyond the end of the sample writes a slab of zeros (the finalizer adds every wave's slab).
//
// trace_wave is the body of all three.  Without apertures a full tile takes the unmasked path and only the last one
// the masked path; with them (LOSSES) every tile is masked.  The order of the branches in the tile loop is the one the
// plain kernels' register allocation was measured with: keep it.
// ---------------------------------------------------------------------------------------
template <typename T, int U, bool LOSSES, bool SCREENS>
__device__ __forceinline__ void trace_wave(const TraceArgs& a, int S, const T* __restrict__ steps, const T* __restrict__ ref,
                                           const T* __restrict__ p_in, T* __restrict__ p_out, double* __restrict__ slabs,
                                           const TraceLosses& loss, const TraceScreens& scr) {
  const int wgs = a.waves / 4;
  const int64_t b = blockIdx.x / wgs;
  const int w = (int)(blockIdx.x - b * wgs) * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int P = S + 1;
  const T* sample_steps = steps + b * (int64_t)S * LYNX_STEP_STRIDE;
  const T* sample_ref = ref + b * (int64_t)P * kTraceRef;
  const T* src = p_in + b * a.in_stride;
  T* dst = p_out + b * a.n_particles * 7;
  double* slab = slabs + (b * a.waves + w) * (int64_t)P * kTraceSlab;
  const T* limits = LOSSES ? static_cast<const T*>(loss.limits) + b * loss.limit_stride : nullptr;
  int32_t* lost_at = LOSSES && loss.lost_at ? loss.lost_at + b * a.n_particles : nullptr;
  constexpr int64_t kTile = 64 * U;
  const int64_t begin = (int64_t)w * a.tiles_per_wave * kTile;
  if (begin >= a.n_particles) {
    for (int64_t i = lane; i < (int64_t)P * kTraceSlab; i += 64) slab[i] = 0.0;
    return;
  }
  for (int t = 0; t < a.tiles_per_wave; ++t) {
    const int64_t base = begin + t * kTile;
    if (base >= a.n_particles) break;
    if constexpr (LOSSES)
      trace_tile<T, U, true, true, SCREENS>(a, S, sample_steps, sample_ref, src, dst, base, lane, t == 0, slab, loss, limits, lost_at, scr, b);
    else if (base + kTile <= a.n_particles)
      trace_tile<T, U, false, false, false>(a, S, sample_steps, sample_ref, src, dst, base, lane, t == 0, slab, loss, limits, lost_at, scr, b);
    else
      trace_tile<T, U, true, false, false>(a, S, sample_steps, sample_ref, src, dst, base, lane, t == 0, slab, loss, limits, lost_at, scr, b);
  }
}

template <typename T, int U>
__global__ __launch_bounds__(256) void k_trace_particles(TraceArgs a, int S, const T* __restrict__ steps,
                                                         const T* __restrict__ ref, const T* __restrict__ p_in,
                                                         T* __restrict__ p_out, double* __restrict__ slabs) {
  trace_wave<T, U, false, false>(a, S, steps, ref, p_in, p_out, slabs, TraceLosses{}, TraceScreens{});
}

// ... with active apertures (TraceLosses)
template <typename T, int U>
__global__ __launch_bounds__(256) void k_trace_particles_losses(TraceArgs a, int S, const T* __restrict__ steps,
                                                                const T* __restrict__ ref, const T* __restrict__ p_in,
                                                                T* __restrict__ p_out, double* __restrict__ slabs,
                                                                TraceLosses loss) {
  trace_wave<T, U, true, false>(a, S, steps, ref, p_in, p_out, slabs, loss, TraceScreens{});
}

// ... with active screens (TraceScreens), and with the apertures of `loss` if there are any
template <typename T, int U>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(sizeof(T) == 4 ? 3 : 4))) void k_trace_particles_screens(TraceArgs a, int S, const T* __restrict__ steps,
                                                                 const T* __restrict__ ref, const T* __restrict__ p_in,
                                                                 T* __restrict__ p_out, double* __restrict__ slabs,
                                                                 TraceLosses loss, TraceScreens scr) {
  trace_wave<T, U, true, true>(a, S, steps, ref, p_in, p_out, slabs, loss, scr);
}

// ---------------------------------------------------------------------------------------
// k_trace_finalize: grid.x = B * P, THREADS = 32 G threads.  The slabs of the sample's waves at this point: group g
// adds the g-th of G contiguous ranges of waves in wave order (one thread per cell), the G sums are added in group
// order -- a fixed association for a given launch plan -- and the record is written as write_moment_record writes
// it: every slab was taken about the same reference point, so there is nothing to move.
// (One group alone: 2608 dependent additions per cell for one sample of 10^6 particles, 577 us -- more than the
// streaming kernel's 122.)
// `count`: the number of particles a record stands for (slot 35), N -- or negative, for a trace with losses: the number
// of particles alive at that point (a point nobody reaches: count 0 and, by write_moment_record's divisions, NaN
// moments).
// ---------------------------------------------------------------------------------------
template <typename T, int THREADS>
__global__ __launch_bounds__(THREADS) void k_trace_finalize(const double* __restrict__ slabs, const T* __restrict__ ref,
                                                            int waves, int P, int64_t count, double* __restrict__ out) {
  constexpr int G = THREADS / kTraceSlab;
  __shared__ double s_part[G][kTraceSlab];
  __shared__ double s[kPartialStride];
  const int tid = threadIdx.x, cellid = tid & (kTraceSlab - 1), g = tid / kTraceSlab;
  const int64_t b = blockIdx.x / P;
  const int k = (int)(blockIdx.x - b * P);
  {
    const int per = (waves + G - 1) / G;
    const int w0 = g * per, w1 = min(waves, w0 + per);
    const double* cell = slabs + ((b * waves) * (int64_t)P + k) * kTraceSlab + cellid;
    double v = 0.0;
#pragma unroll 8
    for (int w = w0; w < w1; ++w) v += cell[(int64_t)w * P * kTraceSlab];
    s_part[g][cellid] = v;
  }
  __syncthreads();
  if (tid < kPartialStride) {
    double v = 0.0;
    if (tid < 28) {
#pragma unroll
      for (int q = 0; q < G; ++q) v += s_part[q][tid];
    } else if (tid < 34) {
      v = (double)ref[(b * P + k) * kTraceRef + (tid - 28)];
    } else if (tid == 34) {
      v = 1.0;
    } else if (count < 0) {  // the point's own count: the sum of the 7th coordinate, exact (integers in float64)
#pragma unroll
      for (int q = 0; q < G; ++q) v += s_part[q][6];
    } else {
      v = (double)count;
    }
    s[tid] = v;
  }
  __syncthreads();
  if (tid < kPartialStride) write_moment_record(s, out + (b * P + k) * kPartialStride, tid);
}

// ---------------------------------------------------------------------------------------
// k_moments_by_loss: the moment records of the INCOMING beam over the nested survivor sets of a trace with losses
// (lynx_moments_by_loss).  Set j holds the particles alive behind the first j apertures: lost_at == -1 or lost_at >= j;
// set 0 is everyone.  The kernel is the particle kernel with identity steps whose "points" are the sets: the same grid
// and wave plan, a tile of 64 U particles in registers with their `lost_at`, per set the 28 shifted sums with a select
// on `lost_at` (trace_point's masked form), the transposing butterfly, the wave's own float64 slab [A + 1][32]; then
// k_trace_finalize in its per-point-count mode.  The reference point of every sum of a sample is the median of the
// candidates (trace_reference_median) that are finite and members of the innermost set any candidate is a member of -- a
// point inside every non-empty set that holds a candidate, wherever the lost particles are.  Every wave works it out for
// itself from `lost_at` (64 loads, the same bits in every wave); wave 0 of a sample writes it where the finalizer looks for
// it, `ref_out` [B][A + 1][kTraceRef].  No atomics, one fixed order.
// ---------------------------------------------------------------------------------------
struct LossSetArgs {
  int64_t n_particles;
  int64_t in_stride;  // scalars between the samples of p_in: N * 7, or 0 for one shared incoming beam
  int32_t waves;      // waves per sample (a multiple of 4)
  int32_t tiles_per_wave;
  int32_t sets;       // A + 1
};

template <typename T, int U>
__device__ __forceinline__ void loss_sets_tile(const LossSetArgs& a, const T* __restrict__ src, const T* __restrict__ ref /* six scalars */,
                                               const int32_t* __restrict__ lost_at, int64_t base, int lane, bool first,
                                               double* __restrict__ slab /* of this wave */) {
  bool inside[U];
  int32_t gone[U];
  T z[U][7];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int64_t i = base + lane + 64 * u;
    inside[u] = i < a.n_particles;
    // (a lane beyond the end of the sample carries the sample's last particle: finite work, no part in any sum)
    const int64_t at = inside[u] ? i : a.n_particles - 1;
    load_particle(src + at * 7, z[u]);
    gone[u] = lost_at[at];
  }
  if constexpr (sizeof(T) == 4) {
    lynx_f32x2 zp[U / 2][7];
#pragma unroll
    for (int u = 0; u < U; u += 2)
#pragma unroll
      for (int c = 0; c < 7; ++c) {
        zp[u / 2][c].x = z[u][c];
        zp[u / 2][c].y = z[u + 1][c];
      }
#pragma nounroll
    for (int j = 0; j < a.sets; ++j) {
      bool live[U];
#pragma unroll
      for (int u = 0; u < U; ++u) live[u] = inside[u] && (gone[u] < 0 || gone[u] >= j);
      trace_point<U, true>(zp, ref, live, lane, first, slab + (int64_t)j * kTraceSlab);
    }
  } else {
#pragma nounroll
    for (int j = 0; j < a.sets; ++j) {
      bool live[U];
#pragma unroll
      for (int u = 0; u < U; ++u) live[u] = inside[u] && (gone[u] < 0 || gone[u] >= j);
      trace_point<U, true>(z, ref, live, lane, first, slab + (int64_t)j * kTraceSlab);
    }
  }
}

template <typename T, int U>
__global__ __launch_bounds__(256) void k_moments_by_loss(LossSetArgs a, const T* __restrict__ p_in,
                                                         const int32_t* __restrict__ lost_at, double* __restrict__ slabs,
                                                         T* __restrict__ ref_out) {
  const int wgs = a.waves / 4;
  const int64_t b = blockIdx.x / wgs;
  const int w = (int)(blockIdx.x - b * wgs) * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int J = a.sets;
  const T* src = p_in + b * a.in_stride;
  const int32_t* gone = lost_at + b * a.n_particles;
  double* slab = slabs + (b * a.waves + w) * (int64_t)J * kTraceSlab;
  constexpr int64_t kTile = 64 * U;
  const int64_t begin = (int64_t)w * a.tiles_per_wave * kTile;
  if (begin >= a.n_particles) {
    for (int64_t i = lane; i < (int64_t)J * kTraceSlab; i += 64) slab[i] = 0.0;
    return;
  }
  T c[6];
  {
    const int64_t at = trace_candidate(lane, a.n_particles);
    T z[7];
    load_particle(src + at * 7, z);
    const int32_t g = gone[at];  // a candidate lost at aperture g is a member of the sets 0 .. g, a survivor of all J
    trace_reference_median<T>(z, trace_finite<T>(z) ? (g < 0 || g >= J ? J : g + 1) : 0, lane, c);
  }
  if (w == 0) {
    T mine = T(0);
#pragma unroll
    for (int k = 0; k < 6; ++k) mine = (lane & (kTraceRef - 1)) == k ? c[k] : mine;
    for (int i = lane; i < J * kTraceRef; i += 64) ref_out[b * J * kTraceRef + i] = mine;  // (64 is a multiple of kTraceRef)
  }
  for (int t = 0; t < a.tiles_per_wave; ++t) {
    const int64_t base = begin + t * kTile;
    if (base >= a.n_particles) break;
    loss_sets_tile<T, U>(a, src, c, gone, base, lane, t == 0, slab);
  }
}

// ---------------------------------------------------------------------------------------
// k_trace_trajectories: the coordinates of K chosen particles at every point.  grid.x = B * ceil(K / (64 U)), 64
// threads: one wave serves one sample and 64 U consecutive CHOSEN particles (float32: U = 2, one packed pair per lane;
// float64: U = 1); chosen particle j of the tile sits in lane j % 64, slot j / 64, like a particle of trace_tile.  No
// LDS, no barrier.  The wave belongs to one sample, so a step's row comes through scalar loads as in trace_tile, and the
// arithmetic is the streaming trace's: apply_step_pair / apply_step<double>, so the last point of a trajectory has the
// bits of the particle kernel's p_out.  At every point the lanes of a slot store 7 scalars each, 28 / 56 bytes apart:
// one contiguous run per wave.
// `plan`: TraceLosses.plan of the call, or null (no apertures, no screens); a screen's code is passed over.  An
// aperture clears `live` by trace_aperture_coded -- the particle kernel's own test -- and writes the chosen particle's
// cell of `lost_in`; a particle that is not alive is stored as NaN in all seven columns: it has its coordinates at the
// point it entered the aperture and none behind it.
// The indices are the host's to check (0 <= index < N); a lane beyond K carries chosen particle K - 1 and stores nothing.
// ---------------------------------------------------------------------------------------
struct TraceTrajectories {
  const int64_t* indices;  // [K]
  int64_t count;           // K >= 1
  void* out;               // [B][P][K][7], lattice dtype
  int32_t* lost_in;        // [B][K], -1 everywhere before the launch; or null
};

template <typename T>
__device__ __forceinline__ void trace_store_chosen(T* __restrict__ dst, const T (&z)[7], bool live) {
  T v[7];
#pragma unroll
  for (int c = 0; c < 7; ++c) v[c] = live ? z[c] : T(__builtin_nanf(""));
  store_particle(dst, v);
}

template <typename T>
__global__ __launch_bounds__(64) void k_trace_trajectories(TraceTrajectories t, int S, const T* __restrict__ steps,
                                                           const T* __restrict__ p_in, int64_t in_stride,
                                                           const int64_t* __restrict__ plan, const T* __restrict__ limits_all,
                                                           int64_t limit_stride) {
  constexpr int U = sizeof(T) == 4 ? 2 : 1;
  constexpr int64_t kTile = 64 * U;
  const int64_t K = t.count, tiles = (K + kTile - 1) / kTile;
  const int64_t b = blockIdx.x / tiles;
  const int64_t base = ((int64_t)blockIdx.x - b * tiles) * kTile;
  const int lane = threadIdx.x, P = S + 1;
  const T* sample_steps = steps + b * (int64_t)S * LYNX_STEP_STRIDE;
  const T* limits = limits_all ? limits_all + b * limit_stride : nullptr;
  int32_t* lost_in = t.lost_in ? t.lost_in + b * K + base : nullptr;
  T* out = static_cast<T*>(t.out) + (b * P * K + base + lane) * 7;  // this lane's first slot at point 0
  bool chosen[U], live[U];
  T z[U][7];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int64_t j = base + lane + 64 * u;
    chosen[u] = live[u] = j < K;
    const int64_t idx = t.indices[chosen[u] ? j : K - 1];
    load_particle(p_in + b * in_stride + idx * 7, z[u]);
  }
  if constexpr (sizeof(T) == 4) {
    lynx_f32x2 zp[7];
#pragma unroll
    for (int c = 0; c < 7; ++c) zp[c] = lynx_f32x2{z[0][c], z[1][c]};
    for (int s = 0; s <= S; ++s) {
#pragma unroll
      for (int c = 0; c < 7; ++c) z[0][c] = zp[c].x, z[1][c] = zp[c].y;
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (chosen[u]) trace_store_chosen<T>(out + ((int64_t)s * K + 64 * u) * 7, z[u], live[u]);
      if (s == S) break;
      if (plan) {
        const int code = __builtin_amdgcn_readfirstlane((int)plan[s]);
        if (code >= 0 && !(code & 1))
          trace_aperture_coded<T, U>(code >> 1, limits, [&](int u, T& x, T& y) {
            x = u ? zp[0].y : zp[0].x;
            y = u ? zp[2].y : zp[2].x;
          }, live, lost_in, lane);
      }
      const T* tab = sample_steps + s * LYNX_STEP_STRIDE;  // global, wave-uniform: scalar loads
      const int desc = (int)uniform_value(tab[LYNX_FLAGS_OFFSET]);
      const int skind = (desc >> LYNX_DESC_KIND_SHIFT) & 3, sflags = desc & 0xffff;
      T m[LYNX_STEP_SCALARS];
#pragma unroll
      for (int q = 0; q < LYNX_STEP_SCALARS; ++q) m[q] = uniform_value(tab[q]);
      apply_step_pair(m, skind, sflags, zp);
    }
  } else {
    for (int s = 0; s <= S; ++s) {
      if (chosen[0]) trace_store_chosen<T>(out + (int64_t)s * K * 7, z[0], live[0]);
      if (s == S) break;
      if (plan) {
        const int code = __builtin_amdgcn_readfirstlane((int)plan[s]);
        if (code >= 0 && !(code & 1))
          trace_aperture_coded<T, U>(code >> 1, limits, [&](int, T& x, T& y) {
            x = z[0][0];
            y = z[0][2];
          }, live, lost_in, lane);
      }
      const T* tab = sample_steps + s * LYNX_STEP_STRIDE;
      const int desc = (int)tab[LYNX_FLAGS_OFFSET];
      const int skind = (desc >> LYNX_DESC_KIND_SHIFT) & 3, sflags = desc & 0xffff;
      apply_step<T>(tab, skind, sflags, z[0]);
    }
  }
}

// ---------------------------------------------------------------------------------------
// ParameterBeam: mu_k = M_k mu_{k-1}, cov_k = M_k cov_{k-1} M_k^T (element.py:71-82), the cavity branch of
// cavity.py:134-140, 202-218 -- the step functions of k_track_moments / k_apply_moments_lanes (moment_step_wave,
// moment_step_lanes in lynx_device.hpp), every intermediate written: mu [B][P][7], cov [B][P][7][7].  (The energies
// come from k_trace_reference.)
//
// k_trace_moments: one wave per sample, 49 lanes busy (moment_step_wave); the table is read from memory.
// ---------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(64) void k_trace_moments(LatticeDev lat, const T* __restrict__ steps,
                                                      const T* __restrict__ mu_in, const T* __restrict__ cov_in,
                                                      T* __restrict__ mu_trace, T* __restrict__ cov_trace) {
  __shared__ T s_mu[8], s_cov[49], s_x[49];
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x, S = lat.n_steps, P = S + 1;
  if (lane < 7) s_mu[lane] = mu_in[b * 7 + lane];
  if (lane < 49) s_cov[lane] = cov_in[b * 49 + lane];
  __syncthreads();
  const int cl = lane < 49 ? lane : 48;
  const int i = cl / 7, j = cl % 7;
  for (int s = 0; s <= S; ++s) {
    if (lane < 7) mu_trace[(b * P + s) * 7 + lane] = s_mu[lane];
    if (lane < 49) cov_trace[(b * P + s) * 49 + lane] = s_cov[lane];
    if (s == S) break;
    const T* M = steps + (b * S + s) * LYNX_STEP_STRIDE;
    const int desc = (int)M[LYNX_FLAGS_OFFSET];
    const bool kick = ((desc >> LYNX_DESC_KIND_SHIFT) & 3) == LYNX_STEP_CAVITY && (desc & LYNX_FLAG_CAV_GAIN);
    moment_step_wave<T>(M, s_mu, s_cov, s_x, lane, i, j, kick);
  }
}

// k_trace_moments_lanes: large float32 batches, lanes = samples (moment_step_lanes: a wave stages the
// 64 table rows of a step in LDS with coalesced loads, every lane propagates its own sample's moments in registers).
template <typename T>
__global__ __launch_bounds__(64) void k_trace_moments_lanes(LatticeDev lat, const T* __restrict__ steps,
                                                            const T* __restrict__ mu_in, const T* __restrict__ cov_in,
                                                            T* __restrict__ mu_trace, T* __restrict__ cov_trace) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  using V = typename VecOf<T, true>::type;
  constexpr int W = VecOf<T, true>::width, kVecPerRow = LYNX_STEP_STRIDE / W;
  T* rows = reinterpret_cast<T*>(smem_raw);
  const int lane = threadIdx.x, S = lat.n_steps, P = S + 1;
  const int64_t b0 = (int64_t)blockIdx.x * 64, B = lat.batch;
  const bool alive = b0 + lane < B;
  const int64_t b = alive ? b0 + lane : B - 1;
  T mu[7], C[49];
#pragma unroll
  for (int q = 0; q < 7; ++q) mu[q] = mu_in[b * 7 + q];
#pragma unroll
  for (int q = 0; q < 49; ++q) C[q] = cov_in[b * 49 + q];
  for (int s = 0; s <= S; ++s) {
    if (alive) {
#pragma unroll
      for (int q = 0; q < 7; ++q) mu_trace[(b * P + s) * 7 + q] = mu[q];
#pragma unroll
      for (int q = 0; q < 49; ++q) cov_trace[(b * P + s) * 49 + q] = C[q];
    }
    if (s == S) break;
    wave_fence();
#pragma unroll 4
    for (int v = lane; v < 64 * kVecPerRow; v += 64) {
      const int r = v / kVecPerRow, piece = v - r * kVecPerRow;
      const int64_t br = (b0 + r < B) ? b0 + r : B - 1;
      const V x = *reinterpret_cast<const V*>(steps + (br * S + s) * LYNX_STEP_STRIDE + piece * W);
      *reinterpret_cast<V*>(rows + r * 68 + piece * W) = x;
    }
    wave_fence();
    const T* M = rows + lane * 68;
    moment_step_lanes<T>(M, mu, C);
  }
}

// ---------------------------------------------------------------------------------------
// The screen images of a ParameterBeam along the trace, their gradients and the image loss: seven kernels on five shared
// pieces, so that all of them see ONE image --
//   trace_screen_state       a sample's ScreenState at a screen: mu, cov of ONE point of the moment trace, mu_x and mu_y
//                            less the screen's misalignment (Screen._observe, formed in the lattice's dtype)
//   gaussian_density         (lynx_device.hpp) the density of a cell, k_gaussian_image's own
//   image_adjoint_add        a cell's part of the six adjoint sums
//   image_block_sums<N>, image_sample_sums<N>   N float64 sums over a workgroup's cells into slab[b][chunk][N], and over a
//                            sample's chunks from there: no atomics, one fixed order of additions
//   image_entries_add        the five entries of mu_bar, cov_bar and the misalignment's gradient from the six sums
// The loss and the gradients are those of the image the forward kernel writes, bit for bit, because there is no second
// copy of any of these expressions to drift.
// ---------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ ScreenState<T> trace_screen_state(const T* __restrict__ mu_trace, const T* __restrict__ cov_trace, int P,
                                                             int point, const T* __restrict__ misalignment /* of this screen */,
                                                             int64_t misalignment_stride, int64_t b) {
  const T* mu = mu_trace + (b * P + point) * 7;
  const T* cov = cov_trace + (b * P + point) * 49;
  const T mx = mu[0] - misalignment[b * misalignment_stride], my = mu[2] - misalignment[b * misalignment_stride + 1];
  const T a = cov[0], bb = cov[2], c = cov[2 * 7 + 2];
  return {mx, my, a, bb, c, a * c - bb * bb};
}

// k_gaussian_image_along: one thread per pixel; the image is [nx][ny] at `image` + b * cells.
template <typename T>
__global__ __launch_bounds__(256) void k_gaussian_image_along(const T* __restrict__ mu_trace, const T* __restrict__ cov_trace,
                                                              int P, int point, const T* __restrict__ xs, const T* __restrict__ ys,
                                                              int nx, int ny, const T* __restrict__ misalignment /* of this screen */,
                                                              int64_t misalignment_stride, T* __restrict__ image, int64_t cells) {
  const int64_t b = blockIdx.y;
  const int64_t pix = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= (int64_t)nx * ny) return;
  const int i = (int)(pix / ny), j = (int)(pix % ny);
  const ScreenState<T> st = trace_screen_state<T>(mu_trace, cov_trace, P, point, misalignment, misalignment_stride, b);
  const T dx = xs[i] - st.mx, dy = ys[j] - st.my;
  image[b * cells + (int64_t)(nx - 1 - i) * ny + j] = gaussian_density<T>(st, dx, dy);
}

// ---------------------------------------------------------------------------------------
// The adjoint of an image: W = dL/d(image) of one screen reduced to six sums per sample,
//   S0 = sum W I, Sx = sum W I ux, Sy = sum W I uy, Sxx = sum W I ux^2, Sxy = sum W I ux uy, Syy = sum W I uy^2,
//   ux = (c dx - b dy) / det, uy = (a dy - b dx) / det  (d log I / d mx, d log I / d my),
// in float64 for both dtypes.  image_adjoint_add adds one cell's part, wi = W I, to s[0 .. 5].
// ---------------------------------------------------------------------------------------
constexpr int kImageGradThreads = 256;
constexpr int kImageGradCells = LYNX_IMAGE_GRAD_CELLS;  // cells one workgroup sums
static_assert(kImageGradCells % kImageGradThreads == 0, "every thread of a workgroup takes as many cells");

template <typename T>
__device__ __forceinline__ void image_adjoint_add(double* s, double wi, const ScreenState<T> st, T dx, T dy) {
  const double ux = (double)((st.c * dx - st.bb * dy) / st.det), uy = (double)((st.a * dy - st.bb * dx) / st.det);
  const double wx = wi * ux, wy = wi * uy;
  s[0] += wi;
  s[1] += wx;
  s[2] += wy;
  s[3] += wx * ux;
  s[4] += wx * uy;
  s[5] += wy * uy;
}

__device__ __forceinline__ double image_grad_wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// The N sums of a workgroup's threads -> slab[b][chunk][N]: across the wave with cross-lane adds, across the four waves,
// 0 .. 3 in that order, through `part` in LDS.  No atomics: image_sample_sums adds a sample's chunks in a fixed order.
template <int N>
__device__ __forceinline__ void image_block_sums(double (&s)[N], double (*part)[N], double* __restrict__ slab, int64_t b, int chunks,
                                                 int chunk, int tid) {
#pragma unroll
  for (int q = 0; q < N; ++q) s[q] = image_grad_wave_sum(s[q]);
  if ((tid & 63) == 0) {
#pragma unroll
    for (int q = 0; q < N; ++q) part[tid >> 6][q] = s[q];
  }
  __syncthreads();
  if (tid < N) {
    double total = part[0][tid];
#pragma unroll
    for (int v = 1; v < kImageGradThreads / 64; ++v) total += part[v][tid];
    slab[(b * chunks + chunk) * N + tid] = total;
  }
}

// ... and of a sample from there, by one wave: lane l adds the chunks l, l + 64, ... in that order, then the lanes are
// added across the wave; every lane has the sums.
template <int N>
__device__ __forceinline__ void image_sample_sums(double (&s)[N], const double* __restrict__ slab, int64_t b, int chunks, int lane) {
#pragma unroll
  for (int q = 0; q < N; ++q) s[q] = 0;
  for (int chunk = lane; chunk < chunks; chunk += 64) {
#pragma unroll
    for (int q = 0; q < N; ++q) s[q] += slab[(b * chunks + chunk) * N + q];
  }
#pragma unroll
  for (int q = 0; q < N; ++q) s[q] = image_grad_wave_sum(s[q]);
}

// The five entries the six sums make at the screen's point, ADDED there, and the misalignment's gradient, written:
//   mu_bar[0] += Sx, mu_bar[2] += Sy, cov_bar[0][0] += (Sxx - c/det S0) / 2, cov_bar[2][2] += (Syy - a/det S0) / 2,
//   cov_bar[0][2] and cov_bar[2][0] += (Sxy + b/det S0) / 2 each (their sum is the derivative by the covariance b),
//   gm[at], gm[at + 1] = (-Sx, -Sy) unless gm is null.
// a, b, c and det in float64 from `cov`; `rounded` takes every float64 value to T the caller's way.
template <typename T, typename Rounded>
__device__ __forceinline__ void image_entries_add(const double* s, const T* cov, T* mb, T* cb, T* gm, int64_t at,
                                                  Rounded rounded) {
  const double a = (double)cov[0], bb = (double)cov[2], c = (double)cov[2 * 7 + 2];
  const double det = a * c - bb * bb;
  mb[0] += rounded(s[1]);
  mb[2] += rounded(s[2]);
  cb[0] += rounded(0.5 * (s[3] - c / det * s[0]));
  cb[2 * 7 + 2] += rounded(0.5 * (s[5] - a / det * s[0]));
  const T cross = rounded(0.5 * (s[4] + bb / det * s[0]));
  cb[2] += cross;
  cb[2 * 7] += cross;
  if (gm) {
    gm[at] = rounded(-s[1]);
    gm[at + 1] = rounded(-s[2]);
  }
}

// k_gaussian_image_along_bwd: W is image_bar, [nx][ny] in the image's own (x-flipped) layout, and no image is read back.
// A workgroup sums kImageGradCells consecutive cells (flat index: coalesced loads of W; i, j come from the cell index).
template <typename T>
__global__ __launch_bounds__(kImageGradThreads) void k_gaussian_image_along_bwd(
    const T* __restrict__ mu_trace, const T* __restrict__ cov_trace, int P, int point, const T* __restrict__ xs,
    const T* __restrict__ ys, int nx, int ny, const T* __restrict__ misalignment /* of this screen */,
    int64_t misalignment_stride, const T* __restrict__ image_bar /* of this screen */, int64_t cells,
    double* __restrict__ slab /* of this screen: [B][chunks][6] */) {
  __shared__ double s_part[kImageGradThreads / 64][6];
  const int64_t b = blockIdx.y;
  const int chunks = gridDim.x, chunk = blockIdx.x, tid = threadIdx.x;
  const int n = nx * ny;
  const ScreenState<T> st = trace_screen_state<T>(mu_trace, cov_trace, P, point, misalignment, misalignment_stride, b);
  const T* w = image_bar + b * cells;
  double s[6] = {0, 0, 0, 0, 0, 0};
  int k = 0;  // (outside the loop: the compiler then lays image_block_sums out behind the cells, as code written out here)
#pragma unroll
  for (; k < kImageGradCells / kImageGradThreads; ++k) {
    const int cell = chunk * kImageGradCells + k * kImageGradThreads + tid;
    if (cell < n) {
      const int row = cell / ny, j = cell - row * ny, i = nx - 1 - row;
      const T dx = xs[i] - st.mx, dy = ys[j] - st.my;
      const T density = gaussian_density<T>(st, dx, dy);
      image_adjoint_add<T>(s, (double)w[cell] * (double)density, st, dx, dy);
    }
  }
  image_block_sums<6>(s, s_part, slab, b, chunks, chunk, tid);
}

// ... and its finishing step, one wave per sample: lane 0 adds the entries as they are, (T)s.
template <typename T>
__global__ __launch_bounds__(64) void k_gaussian_image_along_bwd_finish(const T* __restrict__ cov_trace, int P, int point,
                                                                        const double* __restrict__ slab, int chunks,
                                                                        T* __restrict__ mu_bar, T* __restrict__ cov_bar,
                                                                        T* __restrict__ grad_misalignment /* of this screen, or null */,
                                                                        int64_t grad_misalignment_stride) {
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x;
  double s[6];
  image_sample_sums<6>(s, slab, b, chunks, lane);
  if (lane != 0) return;
  image_entries_add<T>(s, cov_trace + (b * P + point) * 49, mu_bar + (b * P + point) * 7, cov_bar + (b * P + point) * 49,
                       grad_misalignment, b * grad_misalignment_stride, [](double v) { return (T)v; });
}

// ---------------------------------------------------------------------------------------
// k_gaussian_image_along_mse: the mean squared difference of a screen's image to a target, and the six adjoint sums of that
// loss, in ONE pass over the target -- neither the image nor its cotangent exists in memory.  Per cell r = I - target,
// W = 2 r / cells in double, and a seventh sum is kept: L = sum r^2, slab[b][chunk][7].  `target` is this screen's part of
// sample 0's row; sample b's is target_stride further (0: one target for the whole batch, which then stays in cache
// while every sample reads it).
// ---------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kImageGradThreads) void k_gaussian_image_along_mse(
    const T* __restrict__ mu_trace, const T* __restrict__ cov_trace, int P, int point, const T* __restrict__ xs,
    const T* __restrict__ ys, int nx, int ny, const T* __restrict__ misalignment /* of this screen */,
    int64_t misalignment_stride, const T* __restrict__ target /* of this screen */, int64_t target_stride,
    double* __restrict__ slab /* of this screen: [B][chunks][7] */) {
  __shared__ double s_part[kImageGradThreads / 64][7];
  const int64_t b = blockIdx.y;
  const int chunks = gridDim.x, chunk = blockIdx.x, tid = threadIdx.x;
  const int n = nx * ny;
  const ScreenState<T> st = trace_screen_state<T>(mu_trace, cov_trace, P, point, misalignment, misalignment_stride, b);
  const T* t = target + b * target_stride;
  const double scale = 2.0 / (double)n;
  double s[7] = {0, 0, 0, 0, 0, 0, 0};
  int k = 0;  // (outside the loop, as in k_gaussian_image_along_bwd)
#pragma unroll
  for (; k < kImageGradCells / kImageGradThreads; ++k) {
    const int cell = chunk * kImageGradCells + k * kImageGradThreads + tid;
    if (cell < n) {
      const int row = cell / ny, j = cell - row * ny, i = nx - 1 - row;
      const T dx = xs[i] - st.mx, dy = ys[j] - st.my;
      const T density = gaussian_density<T>(st, dx, dy);
      const double r = (double)density - (double)t[cell];
      image_adjoint_add<T>(s, scale * r * (double)density, st, dx, dy);
      s[6] += r * r;
    }
  }
  image_block_sums<7>(s, s_part, slab, b, chunks, chunk, tid);
}

// ... its finishing step, one wave per sample: lane 0 writes sums[b][screen][6] and loss[b][screen] = L / cells.
__global__ __launch_bounds__(64) void k_gaussian_image_along_mse_finish(const double* __restrict__ slab, int chunks, int cells,
                                                                        double* __restrict__ loss /* of this screen */,
                                                                        double* __restrict__ sums /* of this screen */,
                                                                        int n_screens) {
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x;
  double s[7];
  image_sample_sums<7>(s, slab, b, chunks, lane);
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < 6; ++q) sums[b * n_screens * 6 + q] = s[q];
    loss[b * n_screens] = s[6] / (double)cells;
  }
}

// ---------------------------------------------------------------------------------------
// k_gaussian_image_along_mse_apply: the reverse half.  One thread per sample walks the screens in order (two screens never
// race on one point): the entries from sums[b][k], each scaled by loss_bar[b][k] before it is rounded, (T)(bar s).
// A screen without a target has sums of 0: it adds 0 and gets (0, 0), by the same arithmetic.  The screens' points come by
// value, kImageLossScreens of them per launch (screens `first` .. `first + count - 1`); launches follow each other on one
// stream.
// ---------------------------------------------------------------------------------------
constexpr int kImageLossScreens = 64;
struct ImageLossScreens {
  int point[kImageLossScreens];
};

template <typename T>
__global__ __launch_bounds__(64) void k_gaussian_image_along_mse_apply(const T* __restrict__ cov_trace, int64_t B, int P,
                                                                       ImageLossScreens screens, int first, int count,
                                                                       int n_screens, const double* __restrict__ sums,
                                                                       const T* __restrict__ loss_bar, T* __restrict__ mu_bar,
                                                                       T* __restrict__ cov_bar,
                                                                       T* __restrict__ grad_misalignment /* or null */) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  for (int q = 0; q < count; ++q) {
    const int k = first + q, point = screens.point[q];
    const double bar = (double)loss_bar[b * n_screens + k];
    image_entries_add<T>(sums + (b * n_screens + k) * 6, cov_trace + (b * P + point) * 49, mu_bar + (b * P + point) * 7,
                         cov_bar + (b * P + point) * 49, grad_misalignment, (b * n_screens + k) * 2,
                         [bar](double v) { return (T)(bar * v); });
  }
}

}  // namespace lynx

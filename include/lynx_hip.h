/*
 * liblynxhip -- C ABI of the MI355X (gfx950) beam-tracking hot path.
 *
 * This is the drop-in boundary for jank324/lynx's `Segment.track()` path.  The reference
 * has no FFI of its own (it is pure Python on jax.numpy); the functions below are what a
 * binding for that path replaces, and each one cites the reference interface it stands
 * for (paths relative to the reference repository).  Plain pointers and sizes only; every
 * `d_*` pointer is device memory obtained from lynx_buf_alloc.
 *
 * Status convention: every function returns 0 on success and a negative lynx_status on
 * failure; lynx_last_error() returns the message of the last failure on that context.
 */
#ifndef LYNX_HIP_H
#define LYNX_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lynx_ctx lynx_ctx;
typedef struct lynx_lattice lynx_lattice;

enum lynx_status {
  LYNX_OK = 0,
  LYNX_ERR_INVALID = -1, /* bad argument / shape mismatch */
  LYNX_ERR_HIP = -2,     /* HIP runtime error            */
  LYNX_ERR_RCCL = -3,    /* RCCL error                   */
  LYNX_ERR_NOMEM = -4,
  /* a beam reached a cavity with energy <= 0 (or NaN): the reference's `assert Ei > 0` (lynx/accelerator/cavity.py:260).
   * Found on the device while the cavities' whole-batch predicates are evaluated (no read-back per call) and reported
   * by the next call that waits for the GPU anyway: lynx_sync, lynx_buf_d2h.  The Python layer raises AssertionError. */
  LYNX_ERR_ENERGY = -5
};

enum lynx_dtype { LYNX_F32 = 0, LYNX_F64 = 1 };

/* Element kinds on the path (reference: the element modules under lynx/accelerator/). */
enum lynx_kind {
  LYNX_KIND_IDENTITY = 0,   /* Marker (marker.py:32-35), inactive BPM (bpm.py:43-46)   */
  LYNX_KIND_DRIFT = 1,      /* drift.py:44-62               params [L]                 */
  LYNX_KIND_QUADRUPOLE = 2, /* quadrupole.py:66-80          params [L,k1,tilt,mx,my]   */
  LYNX_KIND_DIPOLE = 3,     /* dipole.py:112-181, rbend.py  params [L,angle,e1,e2,tilt,fint,fintx,gap] */
  LYNX_KIND_HCOR = 4,       /* horizontal_corrector.py:52-67 params [L,angle]          */
  LYNX_KIND_VCOR = 5,       /* vertical_corrector.py:52-66  params [L,angle]           */
  LYNX_KIND_CAVITY = 6,     /* cavity.py:97-325             params [L,V,phase_deg,f]   */
  LYNX_KIND_CUSTOM = 7,     /* custom_transfer_map.py:87-88 params [49 map entries]    */
  /* the public helpers of lynx/track_methods.py, exposed as lynx_amd.track_methods */
  LYNX_KIND_BASE_RMATRIX = 8, /* track_methods.py:37-105    params [L,k1,hx,tilt]      */
  LYNX_KIND_ROTATION = 9,     /* track_methods.py:14-34     params [angle]             */
  LYNX_KIND_MISALIGNMENT = 10, /* track_methods.py:108-122  params [mx,my,sign] (sign -1: R_entry, +1: R_exit) */
  LYNX_KIND_SOLENOID = 11,    /* solenoid.py:61-105         params [L,k,mx,my]         */
  LYNX_KIND_UNDULATOR = 12    /* undulator.py:48-60         params [L]                 */
};

/*
 * Whole-batch predicates.  The reference evaluates these as Python `if any(...)` over the
 * whole batch (so they are host decisions there too); the host evaluates them once per
 * lattice and hands them to the kernels as flags.
 */
#define LYNX_FLAG_TILT 1        /* quadrupole: any(tilt != 0)          track_methods.py:101 */
#define LYNX_FLAG_MISALIGNED 2  /* quadrupole: !all(misalignment == 0) quadrupole.py:75    */
#define LYNX_FLAG_THICK 4       /* dipole: any(length != 0)            dipole.py:119        */
#define LYNX_FLAG_CAV_BETA 8    /* cavity: any(V != 0 & E != 0)        cavity.py:290        */
#define LYNX_FLAG_CAV_GAIN 16   /* cavity: any(E + dE > 0)             cavity.py:128        */
#define LYNX_FLAG_CAV_T5XX 32   /* cavity: any(dE > 0)                 cavity.py:164        */

/* One lattice element.  Sample b reads its parameters at
 * pool[param_offset + b * batch_stride + j]; batch_stride == 0 means "same for all samples". */
typedef struct lynx_elem {
  int32_t kind;
  int32_t flags;
  int32_t param_offset;
  int32_t batch_stride;
} lynx_elem;

/* A step of the tracking program = what `Segment.track` calls a "todo"
 * (segment.py:344-354): a maximal run of skippable elements whose maps are composed
 * first (segment.py:329-336), or one active cavity (cavity.py:81-246). */
enum lynx_step_kind { LYNX_STEP_RUN = 0, LYNX_STEP_CAVITY = 1 };
typedef struct lynx_step {
  int32_t kind;  /* lynx_step_kind */
  int32_t first; /* first element index */
  int32_t last;  /* one past the last element index (first+1 for a cavity) */
  int32_t flags; /* cavity steps: copy of the element's LYNX_FLAG_CAV_*; runs: LYNX_STEP_FLAG_RAW */
} lynx_step;
/* Run step: take the first element's map as it is instead of left-multiplying it onto the
 * identity.  `Element.track` applies `transfer_map()` directly (element.py:72,84), while
 * `Segment.transfer_map` starts from eye(7) (segment.py:331-335); the two differ only in
 * signed zeros and in how a NaN entry spreads (NaN * 0).  Cavity steps are always raw
 * (cavity.py:113-121). */
#define LYNX_STEP_FLAG_RAW 64
/* Run step that holds exactly one identity element (an active BPM, bpm.py:48-58): while the particles
 * pass it, the streaming kernel adds up their x and y -- the BPM's reading, `stack([mu_x, mu_y])` of
 * the beam that ENTERS it -- without splitting the pass there.  At most LYNX_MAX_OBSERVERS per
 * program; their sums come back through `d_observations` of lynx_track_particles. */
#define LYNX_STEP_FLAG_OBSERVE 128
#define LYNX_MAX_OBSERVERS 8

/* flags of lynx_track_particles */
#define LYNX_TRACK_MOMENTS 1     /* also accumulate the output-beam moments (fused epilogue) */
#define LYNX_TRACK_TWO_KERNEL 2  /* accepted, no effect: build+compose is always a launch of its own */
/* d_p_in is [N][7]: one incoming beam shared by every sample of the lattice batch.  The
 * reference's `ParticleBeam.broadcast` repeats the particles physically
 * (particle_beam.py:838-843) before a parameter scan; a beam broadcast lazily is read once
 * per sample out of the caches instead, which halves the HBM traffic of the pass. */
#define LYNX_TRACK_SHARED_INPUT 4
/* Apply every step on its own.  By default a run that is followed by an active cavity is applied
 * together with it: one 7x7 application with T_cav . T_run (composed per sample, like the maps
 * of a run are) plus the two rows of T_run that give the s and delta entering the cavity --
 * the same algebra as segment.py:344-354 / cavity.py:113-161, rounded differently. */
#define LYNX_TRACK_SEQUENTIAL_STEPS 8
/* Like LYNX_TRACK_MOMENTS, but accumulate the whole 6x6 covariance (21 products per particle)
 * instead of the second moments the reference's ParticleBeam exposes as properties
 * (particle_beam.py:736-836: the six variances, sigma_xx' and sigma_yy' -- 8 products). */
#define LYNX_TRACK_COVARIANCE 16

/* Layout of one sample's moment record (float64 regardless of the particle dtype):
 * [0..6] mean of the 7 coordinates, [7..27] upper triangle (row-major, i<=j<6) of the
 * BIASED 6x6 covariance, [28..33] reserved (0), [34] 1 if the whole triangle was accumulated,
 * 0 if only the property set was (then every other entry of [7..27] is NaN), [35] number of
 * particles. */
#define LYNX_MOMENT_STRIDE 36

typedef struct lynx_device_info_t {
  char name[64];
  char arch[32];
  int32_t compute_units;
  int32_t lds_bytes_per_cu;
  int64_t hbm_bytes;
} lynx_device_info_t;

/* ---- diagnostics ---------------------------------------------------------------- */
const char* lynx_version(void);
int lynx_device_count(int* count);
int lynx_ctx_create(int device, lynx_ctx** out);
int lynx_ctx_destroy(lynx_ctx* ctx);
const char* lynx_last_error(lynx_ctx* ctx);
int lynx_device_info(lynx_ctx* ctx, lynx_device_info_t* out);
int lynx_sync(lynx_ctx* ctx);
/* HIP-event timer on the context's stream (the stream every kernel below runs on). */
int lynx_timer_start(lynx_ctx* ctx);
int lynx_timer_stop(lynx_ctx* ctx, float* elapsed_ms);
/* Per-launch timing of the streaming kernel (k_track) with HIP events recorded on the
 * context's stream immediately around every launch between begin and end.  This is the
 * figure bench.py's roofline uses; it matches rocprofv3's per-kernel duration. */
int lynx_profile_begin(lynx_ctx* ctx);
int lynx_profile_end(lynx_ctx* ctx, double* total_ms, int64_t* launches);
/* every launch of the profile that lynx_profile_end closed last, in launch order: up to `capacity` durations in
 * milliseconds into ms_out, their number into *launches (bench.py: the per-launch curve of the timed steps) */
int lynx_profile_launches(lynx_ctx* ctx, double* ms_out, int64_t capacity, int64_t* launches);
/* ... and every lynx_gather_moments of that profile: its duration on the stream it ran on (with more than one rank
 * this includes the wait for the slowest rank) */
int lynx_profile_gathers(lynx_ctx* ctx, double* ms_out, int64_t capacity, int64_t* gathers);
/* The launch-plan switches (environment variables LYNX_XPOSE, LYNX_UNROLL, ... -- listed with what each selects at
 * `struct Knobs` in lynx_amd/csrc/lynx_hip.hip) are read ONCE, by lynx_ctx_create; a tracking call reads none.  This
 * reads them again: for tests and A/B scripts that change the environment of a live context.                       */
int lynx_ctx_reload_knobs(lynx_ctx* ctx);

/* Calibration: average time of a plain 16-byte-per-lane copy of `bytes` (read + write),
 * i.e. the practical HBM ceiling of this GPU for a stream shaped like a tracking pass.
 * vec_per_thread: 16-byte vectors each thread copies (a workgroup owns one contiguous block of
 * 256 * vec_per_thread vectors); 0 = grid-stride loop; 100 + n = n per thread with non-temporal
 * stores.  1 is the fastest shape on MI355X (6.2 TB/s, with either kind of store).             */
int lynx_diag_copy(lynx_ctx* ctx, void* d_dst, const void* d_src, size_t bytes, int repeats,
                   int vec_per_thread, float* avg_ms);

/* ---- device buffers (reference: jax.Array storage behind `ParticleBeam.particles`,
 *      particle_beam.py:24-45; the Python side owns the handles) ----------------------- */
int lynx_buf_alloc(lynx_ctx* ctx, size_t bytes, void** d_out);
/* ... for a result the host will read back (what `track` returns of a ParameterBeam: mu, cov -- element.py:71-82; a
 * moment record): small blocks are host memory the GPU writes through, reading them back is a wait and a memcpy */
int lynx_buf_alloc_result(lynx_ctx* ctx, size_t bytes, void** d_out);
int lynx_buf_free(lynx_ctx* ctx, void* d_ptr);
int lynx_buf_h2d(lynx_ctx* ctx, void* d_dst, const void* h_src, size_t bytes);
int lynx_buf_d2h(lynx_ctx* ctx, void* h_dst, const void* d_src, size_t bytes);
int lynx_buf_d2d(lynx_ctx* ctx, void* d_dst, const void* d_src, size_t bytes);
int lynx_buf_memset(lynx_ctx* ctx, void* d_dst, int value, size_t bytes);
int lynx_pool_trim(lynx_ctx* ctx); /* return cached blocks to the driver */

/* ---- lattice program (reference: the `Segment.elements` list and every element's
 *      parameter arrays, segment.py:40-54; partition into steps, segment.py:344-351) --- */
int lynx_lattice_create(lynx_ctx* ctx, int dtype, int64_t batch, int32_t n_elems,
                        const lynx_elem* elems, int32_t n_steps, const lynx_step* steps,
                        const void* pool, int64_t pool_count, lynx_lattice** out);
/* overwrite pool[offset : offset+count] (element parameters changed, e.g. `quad.k1 = ...`) */
int lynx_lattice_update_params(lynx_lattice* lat, int64_t offset, int64_t count, const void* host);
/* overwrite element / step flags (whole-batch predicates that depend on the beam energy) */
int lynx_lattice_set_flags(lynx_lattice* lat, const int32_t* elem_flags, const int32_t* step_flags);
int lynx_lattice_destroy(lynx_lattice* lat);

/* ---- the hot path ----------------------------------------------------------------- */

/* Build every element's 7x7 map from the batched parameters and compose each step's map
 * (reference: Element.transfer_map of every kind, track_methods.py:14-122,
 * Segment.transfer_map segment.py:329-338, Cavity._cavity_rmatrix cavity.py:248-325).
 *   d_energy_in  [B]                      beam energy entering the lattice
 *   d_steps_out  [B][n_steps][64]         per step: 49 map entries + 8 cavity coefficients
 *   d_energy_out [B] or NULL              beam energy leaving the lattice                  */
int lynx_build_compose(lynx_ctx* ctx, lynx_lattice* lat, const void* d_energy_in,
                       void* d_steps_out, void* d_energy_out);

/* Segment.track on a ParticleBeam (reference: segment.py:340-356 -> element.py:83-92
 * `particles @ tm^T`, cavity.py:141-161,219-226).
 *   d_p_in / d_p_out [B][N][7]  (may alias; d_p_in [N][7] with LYNX_TRACK_SHARED_INPUT)
 *   d_energy_in      [B]; may be NULL for a program without steps, unless d_energy_out is given
 *   d_energy_out     [B] or NULL: the beam energy behind the last step (may be d_energy_in); a program without steps
 *                    copies d_energy_in
 *   d_moments_out    [B][36] float64 or NULL (needs LYNX_TRACK_MOMENTS)
 *   d_observations   [B][n_observers][2] float64 or NULL: mean x and mean y of the beam entering
 *                    each LYNX_STEP_FLAG_OBSERVE step, in lattice order (BPM.reading, bpm.py:48-54);
 *                    required when the program has such steps                                 */
int lynx_track_particles(lynx_ctx* ctx, lynx_lattice* lat, int64_t n_particles,
                         const void* d_energy_in, const void* d_p_in, void* d_p_out,
                         void* d_energy_out, double* d_moments_out, int flags, double* d_observations);

/* The allocating form: `Segment.track` returns a NEW beam and leaves the incoming one alone (element.py:75-92), so the
 * blocks of the outgoing beam come from the library's own pool -- one call where the caller of lynx_track_particles
 * makes up to five.  d_out[4]: the particles [B][N][7]; the outgoing energy [B] (only if want_energy_out, else NULL);
 * the moment records [B][36] float64 (only with LYNX_TRACK_MOMENTS / _COVARIANCE); the observations
 * [B][n_observers][2] float64 (only if the program has observer steps).  The caller owns them (lynx_buf_free).
 * On failure nothing is allocated and all four are NULL.                                                          */
int lynx_track_particles_new(lynx_ctx* ctx, lynx_lattice* lat, int64_t n_particles, const void* d_energy_in,
                             const void* d_p_in, int flags, int32_t want_energy_out, void** d_out);

/* Segment.track on a ParameterBeam (reference: element.py:71-82 mu'=T mu, cov'=T cov T^T;
 * cavity.py:134-140,202-218).  d_mu [B][7], d_cov [B][7][7] (in/out may alias).            */
int lynx_track_moments(lynx_ctx* ctx, lynx_lattice* lat, const void* d_energy_in,
                       const void* d_mu_in, const void* d_cov_in, void* d_mu_out,
                       void* d_cov_out, void* d_energy_out);

/* The beam ALONG the lattice: the moment record and the beam energy at the entrance (point 0) and behind every step
 * (point k), from one pass over the particles (reference: the loop of Segment.plot_twiss / plot_twiss_over_lattice,
 * segment.py -- `element.track(beam)` element by element and beta_x, beta_y of every intermediate beam -- and
 * plot_reference_particle_traces; 2 E passes over the particle array there).  The program is expected to hold every
 * element as a step of its own (LYNX_STEP_FLAG_RAW: element.py:72,84 applies the element's map as it is; active
 * cavities as cavity steps, cavity.py:81-246); P = n_steps + 1 points, no limit on n_steps other than memory.
 *   d_p_in           [B][N][7] ([N][7] with LYNX_TRACK_SHARED_INPUT, the only flag)
 *   d_p_out          [B][N][7] or NULL: moments only, half the traffic (may alias d_p_in unless that is shared)
 *   d_energy_trace   [B][P]     beam energy at every point, particle dtype
 *   d_trace_out      [B][P][36] float64 moment records, layout of LYNX_MOMENT_STRIDE, slot 34 = 1 (whole triangle)
 * The sums are taken about a reference point that travels with the beam and added in a fixed order: the same call
 * returns the same bits.  The point is chosen from 64 candidates per sample -- particle 0 and 63 more at equal strides,
 * particle floor(l N / 64) for l = 0 .. 63 --: the component-wise median, at the entrance, of the candidates that are
 * finite there, taken through the same maps.  It is no particle of the beam as a rule.  A record keeps its accuracy
 * wherever the first particle is stored and however far out a minority of the candidates lies; if no candidate is finite
 * at the entrance the point is the origin.
 * This entry point and the three below are one call with or without a list of apertures, of screens and of chosen
 * particles: they refuse the same bad arguments (LYNX_ERR_INVALID, before anything is launched; lynx_last_error starts
 * with "beam trace: ", "beam trace with losses: ", "beam trace with screens: " or "beam trace with trajectories: "),
 * and n_apertures and n_screens are at most 0x1fffffff.                                                               */
int lynx_track_particles_along(lynx_ctx* ctx, lynx_lattice* lat, int64_t n_particles, const void* d_energy_in,
                               const void* d_p_in, void* d_p_out, void* d_energy_trace, double* d_trace_out, int flags);

/* ... with particle losses: steps that are ACTIVE apertures (reference: aperture.py:69-108, which compacts the particle
 * array) clear the particles outside them from every later point instead; nothing is compacted, so samples may lose
 * different numbers of particles.  Arguments as above, and
 *   apertures     host [n_apertures][2]: step index (increasing; the step itself is an identity step of the program),
 *                 1 for an elliptical aperture / 0 for a rectangular one
 *   d_limits      [B][n_apertures][2] (limit_stride = 2 n_apertures) or [n_apertures][2] shared by the batch
 *                 (limit_stride = 0): x_max, y_max in the lattice's dtype
 *   d_lost_at     [B][N] int32 or NULL: ordinal (row of `apertures`) of the aperture that removed the particle, -1 for
 *                 a survivor
 * Aperture k tests the particles that ENTER its step (point `step`), by lynx_aperture_mask's comparison; a particle
 * that fails takes no part in the sums of any later point.  Slot 35 of a record is the number of particles alive at
 * that point; a point with none has count 0 and NaN moments.  d_p_out holds every particle, a lost one as far as the
 * maps took it (possibly inf or NaN).  The reference point is chosen as above from the candidates that stay ALIVE and
 * finite to the last point (each is taken through the steps and the apertures of the call): whether a record is
 * accurate does not depend on the coordinates of particles that are lost before its point.  If no candidate survives
 * to the end, the median of those that live longest is used; the points behind the one where the last of them is lost
 * then have a reference point outside the beam, and float32 records there lose digits as its distance in sigmas grows. */
int lynx_track_particles_along_losses(lynx_ctx* ctx, lynx_lattice* lat, int64_t n_particles, const void* d_energy_in,
                                      const void* d_p_in, void* d_p_out, void* d_energy_trace, double* d_trace_out, int flags,
                                      int32_t n_apertures, const int32_t* apertures, const void* d_limits,
                                      int64_t limit_stride, int32_t* d_lost_at);

/* ... with screens: steps that are ACTIVE screens (reference: screen.py:126-141, 196-213, where the screen swallows the
 * beam and histograms the stored particles on read) count the particles that ENTER them into an image and let them
 * through.  Arguments as above -- n_apertures may be 0: the records are then lynx_track_particles_along's and d_lost_at,
 * if given, is -1 everywhere -- and
 *   screens          host [n_screens][3]: step index (increasing, no aperture's step; the step itself is an identity step
 *                    of the program), nx, ny >= 1 (the image is ny rows of nx pixels)
 *   d_edges          per screen the nx + 1 x edges, then the ny + 1 y edges, in the lattice's dtype (increasing)
 *   d_misalignment   [B][n_screens][2] (misalignment_stride = 2 n_screens) or [n_screens][2] shared by the batch
 *                    (misalignment_stride = 0), lattice dtype; x - misalignment[0] is binned (the reference takes the
 *                    second component off x', screen.py:134-135: no image sees it)
 *   d_images         [B][sum of ny nx] int32, screen after screen: flipud(histogramdd((x, y), edges).T) of the particles
 *                    alive at point `step` -- numpy's bin rule on the very edge values (the last edge belongs to the last
 *                    bin, values outside are dropped), exact integer counts: the same call returns the same bits
 * A particle an aperture has removed is in no later image, whatever its coordinates have become.                      */
int lynx_track_particles_along_screens(lynx_ctx* ctx, lynx_lattice* lat, int64_t n_particles, const void* d_energy_in,
                                       const void* d_p_in, void* d_p_out, void* d_energy_trace, double* d_trace_out, int flags,
                                       int32_t n_apertures, const int32_t* apertures, const void* d_limits,
                                       int64_t limit_stride, int32_t* d_lost_at, int32_t n_screens, const int32_t* screens,
                                       const void* d_edges, const void* d_misalignment, int64_t misalignment_stride,
                                       int32_t* d_images);

/* ... with trajectories: the coordinates of n_chosen CHOSEN particles at every point (reference: the loop of
 * plot_reference_particle_traces, segment.py:387-459 -- `xs[particle]`, `ys[particle]` behind every split element).  A
 * superset of the entry point above: arguments as there, except that n_apertures < 0 and n_screens < 0 mean "no such
 * list" (the call then runs the particle kernel the entry point without that list runs; their pointers are not read), and
 *   n_chosen                >= 1
 *   d_indices               [n_chosen] int64 on the device: 0 <= index < n_particles, any order, repeats allowed, shared
 *                           by the batch.  The caller checks them; the kernel relies on them.
 *   d_trajectories          [B][P][n_chosen][7], lattice dtype: chosen particle j at point k (point 0: as it came in).
 *                           The last point has the bits of d_p_out.  A particle removed by the aperture at step k has its
 *                           coordinates at points <= k and NaN in all seven columns from point k + 1 on.
 *   d_trajectory_lost_in    [B][n_chosen] int32 or NULL: d_lost_at of the chosen particles (ordinal of the aperture
 *                           that removed it, -1 for a survivor)
 * The trajectories are read from d_p_in behind the particle kernel: d_p_out must not alias it.  One more small kernel
 * on the same stream, through the same table and step plan; nothing else of the call changes.  lynx_last_error starts
 * with "beam trace with trajectories: ".                                                                              */
int lynx_track_particles_along_trajectories(lynx_ctx* ctx, lynx_lattice* lat, int64_t n_particles, const void* d_energy_in,
                                            const void* d_p_in, void* d_p_out, void* d_energy_trace, double* d_trace_out, int flags,
                                            int32_t n_apertures, const int32_t* apertures, const void* d_limits,
                                            int64_t limit_stride, int32_t* d_lost_at, int32_t n_screens, const int32_t* screens,
                                            const void* d_edges, const void* d_misalignment, int64_t misalignment_stride,
                                            int32_t* d_images, int64_t n_chosen, const int64_t* d_indices, void* d_trajectories,
                                            int32_t* d_trajectory_lost_in);

/* ... of a ParameterBeam (reference: the same loop; element.py:71-82 mu' = T mu, cov' = T cov T^T per element,
 * cavity.py:134-140,202-218): d_mu_trace [B][P][7], d_cov_trace [B][P][7][7], d_energy_trace [B][P].              */
int lynx_track_moments_along(lynx_ctx* ctx, lynx_lattice* lat, const void* d_energy_in, const void* d_mu_in,
                             const void* d_cov_in, void* d_mu_trace, void* d_cov_trace, void* d_energy_trace);

/* Forward-mode pass of lynx_track_moments_along: the TANGENTS of the moments at EVERY point of the lattice along D
 * directions in parameter space -- few parameters, every output: the orbit response matrix (d centroid at every BPM /
 * d angle of every corrector), the Jacobian of the residuals of a least-squares matching, the curve d beta_x(s) / d k1.
 * The program is the one the trace was made with (every element a step of its own, LYNX_STEP_FLAG_RAW; no limit on the
 * number of elements beyond the trace's own); P = n_steps + 1.  For every direction
 *   mu_dot[0] = 0, C_dot[0] = 0;   mu_dot[k] = M mu_dot[k-1] + Mdot mu[k-1],   C_dot[k] = M C_dot[k-1] M^T + X + X^T,
 *   X = Mdot C[k-1] M^T,   Mdot = sum over the direction's entries at element k - 1 of weight . dM/d(parameter or energy)
 * with mu[k], C[k] read from the forward trace; a step without an entry of the direction takes no Mdot term at all.
 *   d_mu_trace [B][P][7], d_cov_trace [B][P][7][7]   what lynx_track_moments_along wrote (lattice dtype)
 *   the directions, HOST arrays in CSR form: direction d has the entries dir_start[d] .. dir_start[d + 1] - 1
 *     dir_start [n_directions + 1] (dir_start[0] = 0, dir_start[n_directions] = n_entries), dir_leaf [n_entries] the
 *     element, dir_row [n_entries] its parameter row 0 .. 7 (the order of d_grad_params) or 8 for the energy at that
 *     step, dir_weight [n_entries] float64.  Several entries of one direction: an element that occurs several times, a
 *     vector parameter's rows, RBend's angle (which feeds e1 and e2 with weight 1/2), the incoming energy (row 8 at every
 *     leaf, weight 1); two entries on one leaf are added.  A direction without entries gives zeros.
 *   d_mu_dot [B][D][P][7], d_cov_dot [B][D][P][7][7]   float64 for every lattice dtype; entry 6 of mu_dot and row and
 *     column 6 of cov_dot are exact zeros (the 7th coordinate is the constant 1)
 * The derivative conventions are those of the reverse passes (dual evaluation of the map builders).  The sweep's own
 * arithmetic is float64; fixed order, no atomics: the same call returns the same bits.  LYNX_ERR_INVALID before
 * anything is launched (lynx_last_error starts with "beam trace tangents: ") for a null required argument,
 * n_directions < 1, n_entries < 0, a dir_start that does not run from 0 to n_entries without decreasing, an entry whose
 * leaf or row is out of range, a row the element's kind does not have, an empty program, a program that is not the
 * trace's, and a program with a cavity step: behind a cavity the energy, and with it every later map, depends on the
 * cavity's parameters, and a ParticleBeam's moments are not closed under its kick -- left for a later version.       */
int lynx_track_moments_along_forward(lynx_ctx* ctx, lynx_lattice* lat, const void* d_energy_in, const void* d_mu_trace,
                                     const void* d_cov_trace, const int32_t* dir_start, const int32_t* dir_leaf,
                                     const int32_t* dir_row, const double* dir_weight, int32_t n_directions, int32_t n_entries,
                                     double* d_mu_dot, double* d_cov_dot);

/* ... of lynx_track_particles_along: the mean and the biased covariance of the particles obey the same recursion
 * exactly, so the records become the states of the sweep above, on the device, and no pass over the particles is made.
 *   d_trace_fwd [B][P][36] float64   what lynx_track_particles_along wrote
 * Directions, outputs and refusals as above, and LYNX_ERR_INVALID for n_particles < 1.                               */
int lynx_track_particles_along_forward(lynx_ctx* ctx, lynx_lattice* lat, int64_t n_particles, const void* d_energy_in,
                                       const double* d_trace_fwd, const int32_t* dir_start, const int32_t* dir_leaf,
                                       const int32_t* dir_row, const double* dir_weight, int32_t n_directions, int32_t n_entries,
                                       double* d_mu_dot, double* d_cov_dot);

/* ... of a ParameterBeam THROUGH cavity steps: a linac's response matrix.  The two entries above refuse a cavity step;
 * this one walks through it.  A direction carries a tangent of the beam energy, e_dot[k] for the energy that enters
 * step k: e_dot[0] = dir_energy_seed[d] (1 for the incoming energy, else 0), and behind a gaining cavity
 * (LYNX_FLAG_CAV_GAIN) + weight . cos(phi) for an entry on its voltage, - weight . V sin(phi) pi/180 for one on its
 * phase.  The tangent of a step's row -- its map and the 8 cavity coefficients -- is taken at the step's OWN entering
 * energy, and an entry on row 8 (the energy at that step) contributes weight . e_dot[leaf] . d(row)/dE: the host gives
 * such an entry, weight 1, to every leaf behind the first cavity whose voltage or phase a direction holds, and to every
 * leaf for the incoming energy.  Behind the products of a gaining cavity follows the tangent of the cavity branch of
 * lynx_track_moments_along (the kick on the incoming s, delta; C55 restored; the second-order terms in C44, C45, C54),
 * with cos(a) - cos(phi) and sin(a) - sin(phi) formed without cancellation as in the reverse passes.
 *   dir_energy_seed [n_directions]   HOST array, float64
 *   d_energy_dot [B][D][P]           float64: e_dot at every point; every cell is written
 * Everything else -- arguments, outputs, arithmetic, bit-for-bit repeatability -- as lynx_track_moments_along_forward,
 * whose results this entry reproduces on a program without a cavity step.  LYNX_ERR_INVALID (lynx_last_error starts with
 * "beam trace tangents: ") for that entry's refusals other than the cavity step, for a null dir_energy_seed or
 * d_energy_dot, and for an entry on row 1, 2 or 3 (voltage, phase, frequency) of a cavity that is not a cavity step:
 * without voltage the cavity is a drift-like element of a run and its map has no continuous limit there.           */
int lynx_track_moments_along_forward_cavities(lynx_ctx* ctx, lynx_lattice* lat, const void* d_energy_in, const void* d_mu_trace,
                                              const void* d_cov_trace, const int32_t* dir_start, const int32_t* dir_leaf,
                                              const int32_t* dir_row, const double* dir_weight, int32_t n_directions,
                                              int32_t n_entries, double* d_mu_dot, double* d_cov_dot,
                                              const double* dir_energy_seed, double* d_energy_dot);

/* Reverse pass of lynx_track_moments_along: gradient of a scalar function of the moments and the energy at EVERY point
 * of the lattice (the losses written along a beamline: Twiss values at markers, beam sizes below an aperture, the
 * centroid at every BPM) with respect to every element parameter, the incoming energy and the incoming mu and cov.
 * One reverse sweep of the moment recursion with a cotangent injected at every point; the states come from the forward
 * trace, nothing is tracked again.  The program is the one the trace was made with (every element a step of its own,
 * LYNX_STEP_FLAG_RAW), at most 256 elements (LYNX_ERR_INVALID beyond); P = n_steps + 1.
 *   d_mu_trace [B][P][7], d_cov_trace [B][P][7][7]   what lynx_track_moments_along wrote
 *   d_mu_bar [B][P][7], d_cov_bar [B][P][7][7]       dL/d(mu), dL/d(cov) at every point, entry by entry
 *   d_energy_bar [B][P] or NULL                      dL/d(beam energy at every point)
 *   d_grad_params [B][E][8], d_grad_energy_in [B]    as for lynx_track_particles_backward
 *   d_grad_mu_in [B][7], d_grad_cov_in [B][7][7]     dL/d(incoming mu), dL/d(incoming cov)
 * All in the lattice's dtype.  Sums in a fixed order, no atomics: the same call returns the same bits.               */
int lynx_track_moments_along_backward(lynx_ctx* ctx, lynx_lattice* lat, const void* d_energy_in, const void* d_mu_trace,
                                      const void* d_cov_trace, const void* d_mu_bar, const void* d_cov_bar,
                                      const void* d_energy_bar, void* d_grad_params, void* d_grad_energy_in,
                                      void* d_grad_mu_in, void* d_grad_cov_in);

/* ... of lynx_track_particles_along.  Without a kicking cavity every element is an affine map, so the particles' mean
 * and biased covariance obey the ParameterBeam's recursion exactly and the gradient needs no pass over the particles:
 * the records and their cotangents become the states and cotangents of the sweep above, on the device.
 *   d_trace_fwd  [B][P][36] float64   what lynx_track_particles_along wrote
 *   d_grad_trace [B][P][36] float64   [0..6] d/dmean, [7..27] d/dcov upper triangle, an off-diagonal entry counted once
 *                                     (the convention of lynx_track_particles_backward)
 *   d_energy_bar [B][P] or NULL, d_grad_params, d_grad_energy_in: as above (lattice dtype)
 *   d_grad_mean_in [B][7], d_grad_cov_in [B][7][7]   dL/d(mean), dL/d(biased covariance) of the incoming particles
 * LYNX_ERR_INVALID if the program has a cavity step (the moments are not closed under its kick) or more than 256
 * elements.                                                                                                         */
int lynx_track_particles_along_backward(lynx_ctx* ctx, lynx_lattice* lat, int64_t n_particles, const void* d_energy_in,
                                        const double* d_trace_fwd, const double* d_grad_trace, const void* d_energy_bar,
                                        void* d_grad_params, void* d_grad_energy_in, void* d_grad_mean_in,
                                        void* d_grad_cov_in);

/* ... of lynx_track_particles_along on a program WITH cavity steps: behind a kick the moments are no function of the
 * moments in front of it, so the gradient takes a second pass over the particles -- the reverse sweep of
 * lynx_track_particles_backward (forward sweep, every 4th state parked, walk back through the kicks), in which the moment
 * cotangent of EVERY point p gives every particle the cotangent
 *   inj_p(z)[k] = (mu_bar_p[k] + sum_j G_hat_p[k][j] (z[j] - mean_p[j])) / n  (k < 6),   inj_p(z)[6] = mu_bar_p[6] / n,
 * G_hat the symmetric matrix of the triangle cotangent with the diagonal doubled, at the point where the particle has the
 * state the record was taken from.  The records and cotangents are converted once into a table in the lattice's dtype.
 *   d_p_in        [B][N][7], or [N][7] with LYNX_TRACK_SHARED_INPUT (the only flag): the incoming particles of the trace
 *   d_trace_fwd, d_grad_trace [B][P][36] float64, d_energy_bar [B][P] or NULL, d_grad_params [B][E][8],
 *   d_grad_energy_in [B]                        as for lynx_track_particles_along_backward
 *   d_grad_p_in   [B][N][7] or NULL             dL/d(incoming particles), lattice dtype (a shared beam: per sample)
 * There is no gradient with respect to the incoming mean and covariance.  A program without a cavity step is accepted
 * (a second way to the answer of lynx_track_particles_along_backward).  Fixed summation order, no atomics: the same call
 * returns the same bits.  LYNX_ERR_INVALID before anything is launched (lynx_last_error starts with "beam trace gradients
 * with cavities: ") for a null required argument, n_particles < 1, any other flag, an empty program, more than 64 steps
 * (the parked states of the sweep), a program whose sums do not fit the LDS of a workgroup, d_grad_p_in == d_p_in.   */
int lynx_track_particles_along_backward_cavities(lynx_ctx* ctx, lynx_lattice* lat, int64_t n_particles,
                                                 const void* d_energy_in, const void* d_p_in, int flags,
                                                 const double* d_trace_fwd, const double* d_grad_trace,
                                                 const void* d_energy_bar, void* d_grad_params, void* d_grad_energy_in,
                                                 void* d_grad_p_in);

/* The moment records of an INCOMING beam over the nested survivor sets of a trace with losses: set j holds the particles
 * alive behind the first j apertures (d_lost_at == -1 or >= j; set 0 is everyone).  What the reverse pass below starts
 * its per-set recursions from -- one more streaming pass over the incoming particles.
 *   d_p            [B][N][7], or [N][7] with LYNX_TRACK_SHARED_INPUT (the only flag), in `dtype`
 *   d_lost_at      [B][N] int32, as lynx_track_particles_along_losses wrote it
 *   d_records_out  [B][n_apertures + 1][36] float64, layout of LYNX_MOMENT_STRIDE: mean, biased covariance triangle,
 *                  slot 34 = 1, slot 35 = the set's count (exact); a set without particles has count 0 and NaN moments
 * The sums are taken about one reference point per sample -- the component-wise median of those of the 64 candidates of
 * lynx_track_particles_along (particle floor(l N / 64)) that are finite and members of the innermost set any of them is a
 * member of -- and added in a fixed order, no atomics: the same call returns the same bits.  No finite candidate: the
 * origin.  LYNX_ERR_INVALID before anything is launched (lynx_last_error starts with "moments by loss: ") for a null
 * pointer, n_particles < 1, or n_apertures outside 1 .. 15.                                                           */
int lynx_moments_by_loss(lynx_ctx* ctx, int dtype, int64_t batch, int64_t n_particles, const void* d_p, int flags,
                         int32_t n_apertures, const int32_t* d_lost_at, double* d_records_out);

/* ... of lynx_track_particles_along_losses: gradient of a scalar function of the moments of the SURVIVING beam at every
 * point (and of the energy).  The set of survivors is locally constant in the parameters and held fixed (the limits of
 * the apertures get no gradient); on a fixed set the recursion above holds from point 0 on, an aperture step being the
 * identity.  With Z_j the particles alive behind the first j apertures, the record of point p stands for Z_j, j = the
 * number of apertures at steps < p; per set the call propagates the set's incoming mean and covariance through the
 * step table in float64, takes the cotangents of the set's own points (zero elsewhere) and runs the sweep above; the
 * sets' T_bar are added in set order.  Arguments as for lynx_track_particles_along_backward, and
 *   d_trace_fwd    [B][P][36] float64   what lynx_track_particles_along_losses wrote
 *   n_apertures, apertures              host [n_apertures]: the step indices of the active apertures, increasing
 *   d_set_records  [B][n_apertures + 1][36] float64   what lynx_moments_by_loss wrote for the incoming beam and d_lost_at
 * A set without particles (count 0) is skipped: a cotangent on a point nobody reaches counts for nothing.  There is no
 * gradient with respect to the incoming mean and covariance: no single set of particles came in.  One wave per (sample,
 * set), sums in float64 in a fixed order, no atomics: the same call returns the same bits.  LYNX_ERR_INVALID before
 * anything is launched (lynx_last_error starts with "beam trace gradients with losses: ") for a null argument, a cavity
 * step, more than 256 elements, n_apertures outside 1 .. 15, aperture steps that do not increase or are not identity
 * steps of the program.                                                                                               */
int lynx_track_particles_along_backward_losses(lynx_ctx* ctx, lynx_lattice* lat, int64_t n_particles, const void* d_energy_in,
                                               const double* d_trace_fwd, const double* d_grad_trace, const void* d_energy_bar,
                                               int32_t n_apertures, const int32_t* apertures, const double* d_set_records,
                                               void* d_grad_params, void* d_grad_energy_in);

/* ... and of the trajectories of chosen particles (lynx_track_particles_along_trajectories): gradient of a scalar function of
 * the COORDINATES of n_chosen particles at every point -- the clearance of halo particles to an aperture, a single trace of
 * the reference's plot_reference_particle_traces -- together with, or without, the moment cotangents above.  Per chosen
 * particle the reverse recursion of the mean, through a gaining cavity's kick as well: a single trajectory is differentiable
 * where the moments are not.  Arguments as above, and
 *   n_chosen             >= 1
 *   d_trajectories       [B][P][n_chosen][7], lattice dtype: what lynx_track_particles_along_trajectories wrote (every
 *                        particle alive at every point: no active apertures)
 *   d_trajectories_bar   [B][P][n_chosen][7] float64: dL/d(coordinates of chosen particle j at point k)
 *   d_grad_chosen_in     [B][n_chosen][7], lattice dtype: dL/d(incoming coordinates of chosen particle j), every row of a
 *                        repeated index on its own
 * d_trace_fwd, d_grad_trace, d_grad_mean_in and d_grad_cov_in may be NULL, all four: the call then carries no moment
 * cotangent, and only then may the program hold cavity steps.  One more kernel, one wave per sample, that adds into the
 * T_bar of the moment sweep on the same stream; sums in float64 in a fixed order, no atomics: the same call returns the
 * same bits.  LYNX_ERR_INVALID before anything is launched (lynx_last_error starts with "beam trace gradients with
 * trajectories: ") for a null required argument, n_chosen <= 0, moment arguments given in part, more than 256 elements.   */
int lynx_track_particles_along_backward_trajectories(lynx_ctx* ctx, lynx_lattice* lat, int64_t n_particles,
                                                     const void* d_energy_in, const double* d_trace_fwd,
                                                     const double* d_grad_trace, const void* d_energy_bar, void* d_grad_params,
                                                     void* d_grad_energy_in, void* d_grad_mean_in, void* d_grad_cov_in,
                                                     int64_t n_chosen, const void* d_trajectories,
                                                     const double* d_trajectories_bar, void* d_grad_chosen_in);

/* Reverse pass of lynx_track_particles: gradient of a scalar function L of the outgoing
 * beam's moment record with respect to every element parameter and the incoming energy
 * (the reference only claims differentiability, setup.py:14-17,
 * tests/test_differentiable.py).
 *   d_moments_fwd  [B][36] float64  the forward moment record (lynx_track_particles)
 *   d_grad_moments [B][36] float64  dL/d(record): [0..6] d/dmean, [7..27] d/dcov (upper
 *                                   triangle, each off-diagonal entry counted once)
 *   d_grad_params  [B][E][8]        dL/d(parameter j of element e), parameter order of the
 *                                   element kind; unused slots 0; custom maps: 0
 *   d_grad_energy_in [B]            dL/d(incoming energy)
 *   d_grad_p_in    [B][N][7] or NULL dL/d(incoming particle coordinates) (the reference's
 *                                   tests/test_differentiable.py:75-91 differentiates through those)
 *   d_grad_observations [B][n_observers][2] float64 or NULL: dL/d(reading) of the program's observer steps (active
 *                                   BPMs, bpm.py:48-58: the reading is the mean x, y of the beam that enters the BPM)
 * Limits of this version: at most 64 units -- a unit is a step, or in float32 a [run, cavity]
 * pair of steps (every 4th per-particle state is parked in a fixed-size private array during
 * the forward sweep).  Beyond that the call returns LYNX_ERR_INVALID and launches nothing.
 * (Float64 beyond 58 steps: the workgroup keeps its per-step sums at a stride of the 57
 * entries in use instead of 64, so that 64 steps fit 160 KiB of LDS; the sums are the same.) */
int lynx_track_particles_backward(lynx_ctx* ctx, lynx_lattice* lat, int64_t n_particles,
                                  const void* d_energy_in, const void* d_p_in,
                                  const double* d_moments_fwd, const double* d_grad_moments,
                                  void* d_grad_params, void* d_grad_energy_in, void* d_grad_p_in,
                                  const double* d_grad_observations);

/* Reverse pass of lynx_track_moments (ParameterBeam): gradient of a scalar function of the
 * outgoing (mu, cov) with respect to every element parameter, the incoming energy and the
 * incoming mu and cov (the reference's tests/test_differentiable.py:54-72 makes those the
 * leaves).
 *   d_mu_bar [B][7], d_cov_bar [B][7][7]   dL/d(outgoing mu), dL/d(outgoing cov), entry by entry
 *   d_grad_params [B][E][8], d_grad_energy_in [B]   as for lynx_track_particles_backward
 *   d_grad_mu_in [B][7], d_grad_cov_in [B][7][7]    dL/d(incoming mu), dL/d(incoming cov)
 * No limit on n_steps: k_build_bwd deals the steps of the program to its 256 threads in strided
 * loops (several steps per thread beyond 256; it used to serve the first 256 steps only, and
 * the step energies and the energy cotangent of a longer program came out wrong, without an
 * error).  The build of a long program takes shorter chunks of elements so that its step table
 * fits the LDS next to them.  At most 4095 elements per program.                             */
int lynx_track_moments_backward(lynx_ctx* ctx, lynx_lattice* lat, const void* d_energy_in,
                                const void* d_mu_in, const void* d_cov_in, const void* d_mu_bar,
                                const void* d_cov_bar, void* d_grad_params, void* d_grad_energy_in,
                                void* d_grad_mu_in, void* d_grad_cov_in);

/* Moment read-out of an existing ParticleBeam (reference: particle_beam.py:736-836,
 * one fused pass instead of 14 separate reductions).  d_moments_out [B][36] float64;
 * covariance != 0: the whole 6x6 covariance, else the property set (see LYNX_MOMENT_STRIDE). */
int lynx_moments(lynx_ctx* ctx, int dtype, int64_t batch, int64_t n_particles, const void* d_p,
                 double* d_moments_out, int32_t covariance);

/* Screen read-out of a ParticleBeam: per-sample 2-D histogram of (x, y) with the bin edges the
 * caller supplies (reference: screen.py:196-213, `jnp.histogramdd` with `pixel_bin_edges`
 * :107-120, then `flipud(hist.T)`).  Bin of a value v: last edge <= v, the right-most edge
 * included (numpy.histogramdd).  d_image [B][ny][nx] int32 counts, row 0 = highest y; the
 * call clears it first.  d_xedges [nx+1], d_yedges [ny+1] in the particle dtype.            */
int lynx_histogram2d(lynx_ctx* ctx, int dtype, int64_t batch, int64_t n_particles, const void* d_p,
                     const void* d_xedges, const void* d_yedges, int32_t nx, int32_t ny, int32_t* d_image);

/* Screen read-out of a ParameterBeam: density of the bivariate normal of (x, y) on a pixel grid
 * (reference: screen.py:160-195).  d_xs [nx], d_ys [ny] pixel coordinates, d_mu [B][7],
 * d_cov [B][7][7]; d_image [B][nx][ny] with the x axis flipped, as the reference returns it. */
int lynx_gaussian_image(lynx_ctx* ctx, int dtype, int64_t batch, const void* d_mu, const void* d_cov,
                        const void* d_xs, const void* d_ys, int32_t nx, int32_t ny, void* d_image);

/* ... of a ParameterBeam at screens inside a trace: lynx_gaussian_image's formula on mu, cov of point `point` of
 * lynx_track_moments_along's d_mu_trace [B][n_points][7], d_cov_trace [B][n_points][7][7], with mu_x - misalignment[0],
 * mu_y - misalignment[1] (formed in `dtype`).
 *   screens          host [n_screens][3]: point, nx, ny >= 1
 *   d_grid           per screen the nx pixel centres xs, then the ny centres ys
 *   d_misalignment   [B][n_screens][2] (misalignment_stride = 2 n_screens) or [n_screens][2] (misalignment_stride = 0)
 *   d_images         [B][sum of nx ny], screen after screen, each [nx][ny] in lynx_gaussian_image's layout           */
int lynx_gaussian_images_along(lynx_ctx* ctx, int dtype, int64_t batch, int32_t n_points, const void* d_mu_trace,
                               const void* d_cov_trace, int32_t n_screens, const int32_t* screens, const void* d_grid,
                               const void* d_misalignment, int64_t misalignment_stride, void* d_images);

/* The adjoint of lynx_gaussian_images_along: cotangents of the images, reduced over all pixels of every screen of every
 * sample to cotangents of mu and cov at the points the screens observe.  Arguments up to misalignment_stride exactly as for
 * lynx_gaussian_images_along, and
 *   d_images_bar         [B][sum of nx ny] dL/d(image), in that function's image layout (x flipped), lattice dtype
 *   d_mu_bar             [B][n_points][7], read and written: at each screen's point, entries 0 and 2 are added to
 *   d_cov_bar            [B][n_points][7][7], read and written: entries [0][0], [2][2], [0][2] and [2][0] are added to (the
 *                        xy cotangent in two equal halves: their sum is the derivative by the covariance of x and y)
 *   d_grad_misalignment  [B][n_screens][2] or NULL: dL/d(misalignment) per sample, the negative of the mu_bar entries
 * -- what lynx_track_moments_along_backward takes as d_mu_bar, d_cov_bar on the same stream.  With mx = mu_x -
 * misalignment[0], my = mu_y - misalignment[1], a, b, c = cov_xx, cov_xy, cov_yy, det = a c - b^2 and, per pixel, dx = xs[i]
 * - mx, dy = ys[j] - my, I the image (formed anew from mu and cov by the forward kernel's expression; no image is read), W
 * its cotangent, ux = (c dx - b dy) / det, uy = (a dy - b dx) / det:
 *   S0, Sx, Sy, Sxx, Sxy, Syy = sum over the pixels of W I {1, ux, uy, ux^2, ux uy, uy^2}
 *   mu_bar[0] += Sx, mu_bar[2] += Sy, cov_bar[0][0] += (Sxx - c/det S0) / 2, cov_bar[2][2] += (Syy - a/det S0) / 2,
 *   cov_bar[0][2], cov_bar[2][0] += (Sxy + b/det S0) / 2.
 * One pass over d_images_bar: a workgroup sums LYNX_IMAGE_GRAD_CELLS consecutive cells in float64 (both dtypes) and writes
 * its six partial sums to a slab in the context's scratch; a second small kernel adds a sample's slab in a fixed order.  No
 * atomics: the same call returns the same bits.  det <= 0 gives NaN, as it does in the image; an image that has
 * underflowed to 0 gives 0.  LYNX_ERR_INVALID before anything is launched (lynx_last_error starts with "image gradients
 * along the trace: ") for a null required argument, a batch beyond 65535, a bad stride, a screen outside the trace or
 * without pixels, or one of 2^31 - 2048 pixels or more.                                                              */
#define LYNX_IMAGE_GRAD_CELLS 2048
int lynx_gaussian_images_along_backward(lynx_ctx* ctx, int dtype, int64_t batch, int32_t n_points, const void* d_mu_trace,
                                        const void* d_cov_trace, int32_t n_screens, const int32_t* screens,
                                        const void* d_grid, const void* d_misalignment, int64_t misalignment_stride,
                                        const void* d_images_bar, void* d_mu_bar, void* d_cov_bar,
                                        void* d_grad_misalignment);

/* The mean squared difference of the images of lynx_gaussian_images_along to target images, evaluated on the device: no
 * image and no cotangent of one is made or moved.  Arguments up to misalignment_stride exactly as for
 * lynx_gaussian_images_along, and
 *   target_offsets  host [n_screens]: where this screen's target starts in a sample's row of d_targets, -1: no target
 *   d_targets       [B][target_cells] (target_stride = target_cells) or [target_cells] (target_stride = 0: one row shared by
 *                   the batch), lattice dtype, every target [nx][ny] in lynx_gaussian_image's layout (x flipped)
 *   d_loss          [B][n_screens] float64: mean over the screen's pixels of (I - target)^2; 0 for a screen without a target
 *   d_sums          [B][n_screens][6] float64: S0, Sx, Sy, Sxx, Sxy, Syy of lynx_gaussian_images_along_backward for the
 *                   cotangent W = 2 (I - target) / (nx ny) of that loss; 0 for a screen without a target
 * I is formed per pixel by the forward kernel's expression (the loss is that of the image lynx_gaussian_images_along writes,
 * bit for bit), I - target and W in float64.  One pass over the target: a workgroup sums LYNX_IMAGE_GRAD_CELLS consecutive
 * cells in float64 (both dtypes) and writes seven partial sums to a slab in the context's scratch; a second small kernel adds
 * a sample's slab in a fixed order.  No atomics: the same call returns the same bits.  det <= 0 gives a NaN loss and NaN
 * sums; an image that has underflowed to 0 gives the mean of target^2 and sums of 0.  LYNX_ERR_INVALID before anything is
 * launched (lynx_last_error starts with "image loss along the trace: ") for a null required argument, a batch beyond 65535, a
 * misalignment stride that is neither 0 nor 2 n_screens, a target stride that is neither 0 nor at least the cells the
 * offsets name, a screen outside the trace or without pixels, one of 2^31 - 2048 pixels or more, or an offset that is
 * negative and not -1.                                                                                                  */
int lynx_gaussian_images_along_mse(lynx_ctx* ctx, int dtype, int64_t batch, int32_t n_points, const void* d_mu_trace,
                                   const void* d_cov_trace, int32_t n_screens, const int32_t* screens, const void* d_grid,
                                   const void* d_misalignment, int64_t misalignment_stride, const int64_t* target_offsets,
                                   const void* d_targets, int64_t target_stride, double* d_loss, double* d_sums);

/* ... and its reverse half: d_loss_bar [B][n_screens] (lattice dtype), the cotangents of d_loss, times the five entries
 * that lynx_gaussian_images_along_backward forms from d_sums [B][n_screens][6] and d_cov_trace, ADDED into d_mu_bar
 * [B][n_points][7] and d_cov_bar [B][n_points][7][7] at the screens' points (screen after screen per sample: two screens on
 * one point do not race) -- what lynx_track_moments_along_backward takes on the same stream.  d_grad_misalignment
 * [B][n_screens][2] or NULL: -d_loss_bar (Sx, Sy), written; a screen without a target has sums of 0 and gets (0, 0).  The
 * refusals and the message's beginning are those of lynx_gaussian_images_along_mse.                                    */
int lynx_gaussian_images_along_mse_backward(lynx_ctx* ctx, int dtype, int64_t batch, int32_t n_points,
                                            const void* d_cov_trace, int32_t n_screens, const int32_t* screens,
                                            const double* d_sums, const void* d_loss_bar, void* d_mu_bar, void* d_cov_bar,
                                            void* d_grad_misalignment);

/* The loss every tuning loop on a trace writes, evaluated on the device from the states the trace left there: a weighted
 * sum of squared distances of named beam properties at chosen points to target values.  No cotangent array with a point
 * axis is made on the host or moved.  Exactly one of the two state forms is given:
 *   d_records       [B][n_points][36] float64, what lynx_track_particles_along* wrote (d_mu_trace, d_cov_trace NULL), or
 *   d_mu_trace, d_cov_trace   [B][n_points][7], [B][n_points][7][7] in `dtype`, what lynx_track_moments_along wrote
 *                   (d_records NULL)
 *   d_energy_trace  [B][n_points] in `dtype`, the energy at every point
 *   ddof            0 or 1: the records' variances are scaled by n / (n - ddof), n = slot 35 (unused for mu and cov)
 *   target_points   host [n_target_points][2]: point (strictly increasing) and property mask, not 0 -- bit k is property k of
 *                   mu_x mu_xp mu_y mu_yp mu_s mu_p (0..5), sigma_x .. sigma_p (6..11), sigma_xxp sigma_yyp (12, 13),
 *                   emittance_x|y (14, 15), normalized_emittance_x|y (16, 17), beta_x|y (18, 19), alpha_x|y (20, 21),
 *                   energy (22).  The T terms of a sample, T = the set bits of all masks, are ordered by (point, bit).
 *   d_rows          [T][2] (row_stride = 0: one row set shared by the batch) or [B][T][2] (row_stride = 2 T) float64:
 *                   (target, weight) of every term
 *   d_values        [B][T] float64: the value of every term
 *   d_point_loss    [B][n_target_points] float64: sum over a point's terms, in bit order, of weight (value - target)^2
 *   d_loss          [B] float64: a sample's point losses added in point order
 * The value of a term is formed in float64 for both dtypes (float32 states are widened on load; nothing is contracted):
 *   records   s2_c = rec[tri(c, c)] n / (n - ddof), cross_a = rec[tri(a, a + 1)], mu_c = rec[c]
 *   mu, cov   s2_c = max(cov_cc, floor), floor = 1e-20 rounded to `dtype`; cross_a = cov[a][a + 1]
 *   both      sigma_c = sqrt(s2_c), sigma_xxp = cross_0, sigma_yyp = cross_2; per plane a = 0 | 2: q = s2_a s2_(a+1) -
 *             cross_a^2, emittance = sqrt(max(q, tiny)), tiny the smallest normal number of `dtype`, beta = s2_a /
 *             emittance, alpha = -cross_a / emittance, normalized_emittance = emittance gamma sqrt(1 - 1 / gamma^2) with
 *             gamma = energy / 510998.95069 (0 at gamma == 0)
 * -- the expressions grad.trace_property_cotangents differentiates, not the trace's property rounded to `dtype`.  A record
 * with n == ddof gives the inf or NaN of that arithmetic.  One thread per (sample, target point), the target points by
 * value in the kernel arguments, 64 per launch; a second small kernel adds a sample's point losses.  No atomics: the
 * same call returns the same bits.  Between lynx_profile_begin and _end every launch of this entry and of its reverse half
 * is one more entry of lynx_profile_launches.  LYNX_ERR_INVALID before anything is launched (lynx_last_error starts with "moment
 * loss along the trace: ") for a null required argument, both or neither state form, batch, n_points or n_target_points
 * <= 0, a dtype that is neither float32 nor float64, ddof outside 0 .. 1, a point outside the trace or not increasing,
 * a mask that is 0 or has a bit above 22, a row stride that is neither 0 nor 2 T.                                      */
int lynx_moments_along_loss(lynx_ctx* ctx, int dtype, int64_t batch, int32_t n_points, const double* d_records,
                            const void* d_mu_trace, const void* d_cov_trace, const void* d_energy_trace, int32_t ddof,
                            int32_t n_target_points, const int32_t* target_points, const double* d_rows, int64_t row_stride,
                            double* d_values, double* d_point_loss, double* d_loss);

/* ... and its reverse half.  Arguments up to row_stride exactly as for lynx_moments_along_loss, and
 *   d_loss_bar     [B] float64: the cotangents of d_loss
 *   d_grad_trace   [B][n_points][36] float64, read and written (records form; d_mu_bar, d_cov_bar NULL): dL/d(record), an
 *                  off-diagonal entry counted once -- what lynx_track_particles_along_backward* take
 *   d_mu_bar, d_cov_bar   [B][n_points][7], [B][n_points][7][7] in `dtype`, read and written (mu, cov form; d_grad_trace
 *                  NULL): entry by entry -- what lynx_track_moments_along_backward takes
 *   d_energy_bar   [B][n_points] in `dtype`, read and written; may be NULL if no term is energy or normalized_emittance_*
 * Per sample and term the bar is d_loss_bar[b] 2 weight (value - target), the value recomputed by the forward kernel's
 * expression (the same bits), taken through the rule of grad.trace_property_cotangents (derivative 0 where s2 or q is
 * clamped) and ADDED at the term's point: mu_<c> into slot c; sigma_<c> into the variance of c; sigma_xxp | yyp into the (a,
 * a + 1) entry; emittance, normalized_emittance, beta and alpha of a plane into its two variances and its (a, a + 1)
 * entry -- slots tri(c, c), tri(a, a + 1) of a record, cov_bar[c][c], cov_bar[a][a + 1] --; energy and
 * normalized_emittance into d_energy_bar.  Nothing else is touched.  One thread per (sample, target point) accumulates
 * its point's bars in float64 registers and does one read-add-write per touched entry (mu_bar, cov_bar, energy_bar
 * rounded once, on the add); target points are distinct, so there are no atomics and the same call returns the same
 * bits.  The refusals and the message's beginning are those of lynx_moments_along_loss, and: cotangents of the other
 * state form, a NULL d_energy_bar with a term that depends on the energy.                                              */
int lynx_moments_along_loss_backward(lynx_ctx* ctx, int dtype, int64_t batch, int32_t n_points, const double* d_records,
                                     const void* d_mu_trace, const void* d_cov_trace, const void* d_energy_trace, int32_t ddof,
                                     int32_t n_target_points, const int32_t* target_points, const double* d_rows,
                                     int64_t row_stride, const double* d_loss_bar, double* d_grad_trace, void* d_mu_bar,
                                     void* d_cov_bar, void* d_energy_bar);

/* Test hook: the float32 sine / cosine the cavity kick uses on the device (cavity.py:141-161
 * calls cos per particle), scalar (packed = 0) or two-per-lane (packed = 1) code path.        */
int lynx_diag_phase_trig(lynx_ctx* ctx, int64_t n, const float* d_x, int32_t packed, float* d_sin,
                         float* d_cos);

/* Aperture (reference: aperture.py:69-108): particles with |x| < x_max and |y| < y_max
 * (rectangular) or x^2/x_max^2 + y^2/y_max^2 <= 1 (elliptical) survive.
 *   d_x_max, d_y_max [B] (param_stride 1) or one value for all samples (param_stride 0)
 *   d_mask [B][N] uint8, d_counts / d_offsets [B][ceil(N/1024)], d_totals [B] survivors     */
int lynx_aperture_mask(lynx_ctx* ctx, int dtype, int64_t batch, int64_t n_particles, const void* d_p,
                       const void* d_x_max, const void* d_y_max, int32_t param_stride, int32_t elliptical,
                       unsigned char* d_mask, int32_t* d_counts, int64_t* d_offsets, int64_t* d_totals);
/* One sample: d_kept [total][7] survivors and d_lost [N - total][7] lost particles, each in
 * their original order (what `particles[mask]` returns), from the mask and offsets above.    */
int lynx_aperture_compact(lynx_ctx* ctx, int dtype, int64_t n_particles, const void* d_p,
                          const unsigned char* d_mask, const int64_t* d_offsets, void* d_kept,
                          void* d_lost);

/* Seeded synthetic beam, generated in HBM: uncorrelated 6-D Gaussian per sample, 7th
 * coordinate 1 (shape of ParticleBeam.from_parameters, particle_beam.py:144-170; not the
 * same random stream).  mu[6], sigma[6] are host arrays.                                   */
int lynx_fill_gaussian(lynx_ctx* ctx, int dtype, int64_t batch, int64_t n_particles,
                       const double* mu, const double* sigma, uint64_t seed, void* d_p);

/* Seeded correlated 6-D Gaussian beam, generated in HBM: sample b has its own mean and covariance factor.
 *   d_rows [B][27] float64 on the device: m[0..5], then the lower triangle of the 6x6 factor L row by row
 *          (L00, L10, L11, L20, ... L55); the sample's covariance is L L^T
 * Column c < 6 of particle i of sample b is m[c] + sum_{j <= c} L[c][j] z_j, summed in float64 from j = 0 upwards and
 * rounded once to the dtype; z_j is the normal lynx_fill_gaussian draws for flat scalar (b N + i) 7 + j (so a diagonal
 * L with the same row for every sample gives lynx_fill_gaussian's bits).  Column 6 is 1.                            */
int lynx_fill_gaussian_rows(lynx_ctx* ctx, int dtype, int64_t batch, int64_t n_particles, const double* d_rows,
                            uint64_t seed, void* d_p);

/* Per-sample affine rescale of a beam (ParticleBeam.transformed_to, particle_beam.py:580-715), device to device:
 *   out[b][i][c] = (in[b][i][c] - old_mu[b][c]) / old_sigma[b][c] * new_sigma[b][c] + new_mu[b][c]   (c < 6; column 6 is 1)
 * in the dtype, in this order.
 *   d_rows [B][24] of the dtype: old_mu[6], old_sigma[6], new_sigma[6], new_mu[6]
 *   in_sample_stride (scalars): n_particles * 7, or 0 for one stored sample that every output sample reads
 * d_p_out may be d_p_in unless the stride is 0.                                                                     */
int lynx_transform_particles(lynx_ctx* ctx, int dtype, int64_t batch, int64_t n_particles, const void* d_p_in,
                             int64_t in_sample_stride, const void* d_rows, void* d_p_out);

/* ---- multi-GPU: one process per GPU, RCCL over xGMI (no reference counterpart: the
 *      reference is single-process; batch samples are independent, so only the
 *      per-sample moment records are exchanged) --------------------------------------- */
#define LYNX_UNIQUE_ID_BYTES 128
int lynx_comm_unique_id(char* id_out /* LYNX_UNIQUE_ID_BYTES */);
int lynx_comm_init(lynx_ctx* ctx, int n_ranks, int rank, const char* id);
int lynx_comm_destroy(lynx_ctx* ctx);
/* what the communicator actually is: RCCL version code (ncclGetVersion), ranks, this rank; ranks = 0 when there is none */
int lynx_comm_info(lynx_ctx* ctx, int32_t* rccl_version, int32_t* n_ranks, int32_t* rank);
/* all-gather `count` float64 per rank: d_recv [n_ranks][count].  Asynchronous: it starts when everything issued
 * so far has run -- with more than one rank on a communication stream of its own, underneath the next tracking
 * call (nothing on the main stream waits for it; environment LYNX_GATHER_OVERLAP=0: in line on the main stream,
 * also the default of a one-rank communicator); lynx_buf_d2h and lynx_sync wait for it either way.  Both blocks
 * may be handed to lynx_buf_free at any time: the library keeps them out of its allocator until the gather is done. */
int lynx_gather_moments(lynx_ctx* ctx, const double* d_send, double* d_recv, int64_t count);

#ifdef __cplusplus
}
#endif
#endif /* LYNX_HIP_H */

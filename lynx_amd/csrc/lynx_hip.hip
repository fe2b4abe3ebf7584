// liblynxhip: C-ABI entry points (include/lynx_hip.h) over the gfx950 kernels in
// lynx_device.hpp.  One lynx_ctx per GPU and per process: one HIP stream, a caching
// device allocator (so that `track()` never pays hipMalloc on the hot path), the
// moment-reduction scratch and, optionally, an RCCL communicator.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "lynx_device.hpp"
#include "lynx_grad.hpp"
#include "lynx_units.hpp"
#include "lynx_grad_units.hpp"
#include "lynx_trace.hpp"
#include "lynx_trace_grad.hpp"
#include "lynx_trace_jvp.hpp"
#include "lynx_moment_loss.hpp"

using namespace lynx;

// Launch-plan switches.  The planner picks a form of the computation by shape (wave tiles or per-particle accesses,
// particles per lane, which stream builds and reduces, ...); every knob forces one of the forms it would otherwise pick
// for another shape, for tests (test_every_kernel_variant_gives_the_default_answer) and the A/B scripts under
// scripts/gpu/.  They are read from the environment ONCE, when the context is created (lynx_ctx_reload_knobs reads them
// again); a `track` call reads none.  -1 = not set: the planner decides.
struct Knobs {
  int xpose = -1;             // LYNX_XPOSE             wave tiles through LDS (1) / per-particle accesses (0)
  int unroll = -1;            // LYNX_UNROLL            particles per lane: 1 | 2 | 4
  int mom = -1;               // LYNX_MOM               moment accumulation mode of the float32 kernels: 2 | 3
  int min_tiles_per_wg = -1;  // LYNX_MIN_TILES_PER_WG
  int async_build = -1;       // LYNX_ASYNC_BUILD       build on the second stream (1) / in line (0)
  int side_reduce = -1;       // LYNX_SIDE_REDUCE       moment reduction on the side stream (1) / in line (0)
  int build_host_wait = -1;   // LYNX_BUILD_HOST_WAIT   the host (1) / the main stream (0) waits for an asynchronous build (kept: the host's wait is live from 128 MB per call; tests reach it at a small shape)
  int gather_overlap = -1;    // LYNX_GATHER_OVERLAP    RCCL gather on the side stream (1) / in line (0)
  int lanes_build_min_batch = 256;  // LYNX_LANES_BUILD_MIN_BATCH  lanes = samples build from this batch on
  int piece = 8;              // LYNX_PIECE             elements per piece of the lanes build (kept: 1 and 3 make short lattices grow the pair tree that long ones have; tests)
  int pair_levels_fused = 1;  // LYNX_PAIR_LEVELS_FUSED narrow pair trees in one launch (wide ones always take one per level; kept: 0 is the per-level path deep trees take, reached by tests at a small shape)
  int merge_steps = 1;        // LYNX_MERGE_STEPS       [run, cavity] pairs as one unit
  int reduce_ticket = 1;      // LYNX_REDUCE_TICKET     samples with more records than one workgroup walks: both levels in one launch (0: two launches; kept: the only independent association the ticket kernel is cross-checked against)
  int one_round = -1;         // LYNX_ONE_ROUND         at most this many workgroups per CU in a launch (0: no cap; default: 3 for single-map launches of a few rounds)
  int track_units = 1;        // LYNX_TRACK_UNITS       structured step loop (2: insist)
  int unit_pairs = 1;         // LYNX_UNIT_PAIRS        lattices of merged [run, cavity] pairs of class U: the kernel written for that form (0: the general one, 2: insist)
  int bwd_units = 1;          // LYNX_BWD_UNITS         structured reverse pass (2, for tests: every odd sample is left to the dense kernel all the same)
  int bwd_merge = 1;          // LYNX_BWD_MERGE         merged pairs in the reverse pass
  int bwd_pairs = 1;          // LYNX_BWD_PAIRS         two particles per lane in the float32 reverse pass
  int build_in_tail = 1;      // LYNX_BUILD_IN_TAIL     start the next build in the tail of the streaming kernel
  int small_inline = -1;      // LYNX_SMALL_INLINE      short calls: build, stream and reduce back to back on ONE stream, no events
  int bwd_reuse_table = 1;    // LYNX_BWD_REUSE_TABLE   the reverse pass reads the step table the forward call just built (0: builds its own)
  int host_visible_records = 1;  // LYNX_HOST_VISIBLE_RECORDS  moment records of a few samples in host memory the GPU writes through (0: device memory)
  int alternate_order = 1;    // LYNX_ALTERNATE_ORDER   long calls walk the batch forwards and backwards in turn (0: always forwards, 2: every call backwards)
  int inline_pool = 1;        // LYNX_INLINE_POOL       small lattices: the parameters by value in the kernel arguments (0: always from memory)
};

static void load_knobs(Knobs* k) {
  *k = Knobs();
  const struct { const char* name; int* value; } table[] = {
      {"LYNX_XPOSE", &k->xpose}, {"LYNX_UNROLL", &k->unroll}, {"LYNX_MOM", &k->mom},
      {"LYNX_MIN_TILES_PER_WG", &k->min_tiles_per_wg}, {"LYNX_ASYNC_BUILD", &k->async_build},
      {"LYNX_SIDE_REDUCE", &k->side_reduce}, {"LYNX_BUILD_HOST_WAIT", &k->build_host_wait},
      {"LYNX_GATHER_OVERLAP", &k->gather_overlap}, {"LYNX_LANES_BUILD_MIN_BATCH", &k->lanes_build_min_batch},
      {"LYNX_PIECE", &k->piece}, {"LYNX_PAIR_LEVELS_FUSED", &k->pair_levels_fused},
      {"LYNX_MERGE_STEPS", &k->merge_steps},
      {"LYNX_REDUCE_TICKET", &k->reduce_ticket}, {"LYNX_TRACK_UNITS", &k->track_units}, {"LYNX_ONE_ROUND", &k->one_round}, {"LYNX_UNIT_PAIRS", &k->unit_pairs}, {"LYNX_BWD_UNITS", &k->bwd_units},
      {"LYNX_BWD_MERGE", &k->bwd_merge}, {"LYNX_BWD_PAIRS", &k->bwd_pairs}, {"LYNX_BUILD_IN_TAIL", &k->build_in_tail},
      {"LYNX_SMALL_INLINE", &k->small_inline}, {"LYNX_INLINE_POOL", &k->inline_pool}, {"LYNX_ALTERNATE_ORDER", &k->alternate_order}, {"LYNX_HOST_VISIBLE_RECORDS", &k->host_visible_records}, {"LYNX_BWD_REUSE_TABLE", &k->bwd_reuse_table}};
  for (const auto& t : table) {
    const char* v = getenv(t.name);
    if (v && *v) *t.value = atoi(v);
  }
}
static inline int knob(int value, int dflt) { return value >= 0 ? value : dflt; }

// A buffer of the library's own, grown on demand (ensure_scratch) and reused in stream order.
struct Scratch {
  void* buf = nullptr;
  size_t bytes = 0;
};

struct lynx_ctx {
  Knobs knobs;
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t s_build = nullptr;  // second stream for k_build (BuildOrder)
  static constexpr int kTableSlots = 3;
  hipEvent_t ev_built[kTableSlots] = {};
  // Who waits for whom before a build.  The map build of a `track` call depends on the lattice and the
  // incoming energy only, so it runs on a second stream underneath the previous call's streaming kernel:
  //   s_build:  [wait: table slot free] k_build(n) -> table[n % kTableSlots]   record ev_built
  //   host   :  waits for ev_built (LYNX_BUILD_HOST_WAIT=0: the main stream does, with a barrier packet)
  //   stream :  k_track_direct(n)                                              ev_streamed rides on its dispatch
  // With three table slots the build of call n+1 may start as soon as the streaming kernel of call n-2 has finished,
  // i.e. it runs underneath kernel n-1 and the host, which waits for it, stays two calls ahead of the GPU.
  // Every build is followed at once by the main stream's wait on it, so anything enqueued on the
  // main stream later (copies, other kernels, lynx_sync) is ordered after every build so far.  The
  // build stream in turn waits for the main stream when (a) it reuses a table slot (ev_streamed) or
  // (b) the main stream may have written what the build reads (`main_dirty`, `main_wrote`, `slot_wrote`).
  // The methods are the only code that reads or writes the members (the context makes and destroys the events with its
  // others: make_sync_events, lynx_ctx_destroy).
  struct BuildOrder {
    hipEvent_t ev_streamed_own[kTableSlots] = {}, ev_mark = nullptr;
    hipEvent_t ev_streamed[kTableSlots] = {};  // the slot's current "streamed" event: its own, or a profiled launch's
    bool streamed_valid[kTableSlots] = {};
    // The main stream has enqueued a write that a later build on s_build could read as its incoming energy or its
    // parameter pool, and nothing has waited for it (h2d copies wait themselves; a streaming kernel's outgoing energy
    // is `main_wrote` / `slot_wrote`).  Writes no build can read -- images, masks, moment records, fresh beams -- do not
    // count: marking them would put an ev_mark record and wait into pipelines that have none.
    bool main_dirty = false;
    const void* main_wrote = nullptr;   // energy buffer the last streaming kernel published on the main stream
    // ... and the one each table slot's streaming kernel published: a build that reads the energy of a call further back
    // than the last one (up = U(beam); x = A(beam); y = B(up)) waits for that slot's ev_streamed.  Kernels kTableSlots
    // calls back have been waited for with the slot itself; a wait for the whole main stream (ev_mark) clears them all.
    const void* slot_wrote[kTableSlots] = {};

    // the main stream enqueued a write a build may read (main_stream_writes, kFeedsBuild)
    void main_wrote_build_input() { main_dirty = true; }
    // the event a streaming kernel that reads the table in `slot` carries as its stop event
    hipEvent_t stop_event(int slot) const { return ev_streamed_own[slot]; }
    // A streaming kernel was enqueued that read the table in `slot` (-1: none) and writes `energy_out` (may be null).
    // `stop`: what rides on its dispatch.  A call whose build ran on the main stream (`async` false) carries none --
    // it costs host time: BASELINE config 2 is bound by the host's enqueue rate -- and marks the main stream dirty
    // instead, which makes the next asynchronous build wait for everything enqueued here.
    void streamed(int slot, bool async, hipEvent_t stop, const void* energy_out) {
      if (slot >= 0) {
        ev_streamed[slot] = stop;
        streamed_valid[slot] = async && stop != nullptr;
        if (!async) main_dirty = true;
        slot_wrote[slot] = energy_out;
      }
      if (energy_out) main_wrote = energy_out;  // a later build that reads it must wait for this kernel
    }
    // The table in `slot` has been read on `main` up to here (a reverse pass that reads the forward call's table): the
    // slot's next build waits for this, too.
    hipError_t read_until_here(int slot, hipStream_t main) {
      const hipError_t e = hipEventRecord(ev_streamed_own[slot], main);
      if (e != hipSuccess) return e;
      ev_streamed[slot] = ev_streamed_own[slot];
      streamed_valid[slot] = true;
      return hipSuccess;
    }
    // Orders a build on `bs` into `slot` that reads the energy `energy` behind what it depends on, in this order: the
    // streaming kernel that last read the slot; the tail of the streaming kernel before the one enqueued last
    // (`tail_flag` reaching `tail_value`; null: no such wait); and what the main stream may have written of its inputs.
    hipError_t order_build(hipStream_t bs, hipStream_t main, int slot, const void* energy, unsigned int* tail_flag,
                           uint32_t tail_value) {
      hipError_t e = hipSuccess;
      // the table slot was last read by the streaming kernel kTableSlots calls ago
      if (streamed_valid[slot] && (e = hipStreamWaitEvent(bs, ev_streamed[slot], 0)) != hipSuccess) return e;
      // ... and the build starts in the TAIL of the streaming kernel before the one enqueued last (which has the GPU
      // to itself when it gets there), not at that kernel's head
      if (tail_flag && (e = hipStreamWaitValue32(bs, tail_flag, tail_value, hipStreamWaitValueGte, 0xffffffffu)) != hipSuccess)
        return e;
      // what the build reads (energy, lattice pool) may have been written on the main stream
      if (main_dirty || (main_wrote && main_wrote == energy)) {
        if ((e = hipEventRecord(ev_mark, main)) != hipSuccess || (e = hipStreamWaitEvent(bs, ev_mark, 0)) != hipSuccess) return e;
        main_dirty = false;
        main_wrote = nullptr;
        for (const void*& w : slot_wrote) w = nullptr;
      } else {
        // ... by a streaming kernel further back than the last one: the tail flag says that kernel's last workgroups have
        // been dispatched, not that they have written the energy
        for (int i = 0; i < kTableSlots; ++i)
          if (i != slot && slot_wrote[i] == energy && energy && streamed_valid[i] &&
              (e = hipStreamWaitEvent(bs, ev_streamed[i], 0)) != hipSuccess)
            return e;
      }
      return hipSuccess;
    }
    // No stop event may be waited for any more (they are about to be destroyed, or both streams are idle).
    void forget_stop_events() {
      for (bool& v : streamed_valid) v = false;
    }
  } order;
  unsigned seq = 0;
  // Nothing enqueued on the main stream since the host last waited for it.  Kept by the library itself (set by
  // sync_main, cleared by every entry point that enqueues): asking the runtime -- hipStreamQuery -- puts a marker
  // packet into the queue whose release costs the next kernel ~5 us behind a kernel that left dirty lines in L2.
  bool main_idle = true;
  bool plain_events = false;  // events with HIP's default (system-scope) fence: jobs of more than one rank
  unsigned long_calls = 0;    // streaming launches of 256 MB and more so far (TrackArgs::reversed)
  // The step table (and unit records) the latest forward call built, for a reverse pass that follows it directly on the
  // same lattice, incoming energy and merge form: it reads them instead of building its own (BASELINE config 5: 80 us
  // of 2.27 ms).  Every forward call with steps takes a slot of the ring and leaves its table here (track_table): there
  // is no forward form without one.  Good while no later call has taken a table slot (`seq`), the lattice has not been
  // written to (`version`) and no entry point that writes device memory on the caller's behalf has run since.
  struct FwdTable {
    const lynx_lattice* lat = nullptr;
    uint64_t version = 0;
    const void* energy = nullptr;
    int slot = -1;
    int merged = 0;
    bool units = false;
    size_t energy_bytes = 0;
    unsigned seq = 0;
    bool valid = false;
    // device memory [dst, dst + bytes) is about to be written on the caller's behalf
    void written(const void* dst, size_t bytes) {
      const char *a = (const char*)dst, *e = (const char*)energy;
      if (valid && a < e + energy_bytes && a + bytes > e) valid = false;
    }
    // a forward call has built the table in `slot_` (call number `seq_`) from the energies [energy_in, + energy_bytes_)
    void leave(const lynx_lattice* lat_, uint64_t version_, const void* energy_in, size_t energy_bytes_, const void* energy_out,
               int slot_, int merged_, bool units_, unsigned seq_) {
      lat = lat_;
      version = version_;
      energy = energy_in;
      energy_bytes = energy_bytes_;
      slot = slot_;
      merged = merged_;
      units = units_;
      seq = seq_;
      valid = energy_out != energy_in;  // (a call that overwrites its own incoming energy leaves nothing to come back to)
    }
  } fwd_table;
  std::mutex mu;                     // allocator maps and fwd_table: finalizers may run on other threads
  // every entry point that writes device memory on the caller's behalf says so here, under the lock
  void wrote(const void* dst, size_t bytes) {
    if (!dst || bytes == 0) return;
    std::lock_guard<std::mutex> lock(mu);
    fwd_table.written(dst, bytes);
  }
  hipEvent_t ev_start = nullptr, ev_stop = nullptr;
  // host-mapped status words the kernels can raise a flag in (k_cavity_flags: energy <= 0 at a cavity); the host
  // looks at them whenever it has waited for the GPU anyway
  int32_t* h_status = nullptr;
  int32_t* d_status = nullptr;
  // "streaming kernel k has reached its tail" (TrackArgs.tail_*): the word the kernels write, and how many have been
  // launched with it
  unsigned int* d_tail_flag = nullptr;
  uint32_t tail_seq = 0;
  int can_wait_value = 0;
  std::string err;
  hipDeviceProp_t prop;
  // caching allocator: size class -> free blocks; live pointer -> size class
  std::multimap<size_t, void*> free_blocks;
  std::unordered_map<void*, size_t> live;
  std::vector<std::pair<const char*, size_t>> host_ranges;  // the host-visible blocks there are (live or cached)
  static constexpr int kTableBwd = kTableSlots, kTablePb = kTableSlots + 1, kTableTrace = kTableSlots + 2;
  static constexpr int kPartialRing = 4;
  // Internal scratch (grown on demand, stream-ordered reuse).  Nothing but Scratch members: lynx_ctx_destroy walks the
  // struct as the array of them it is, so a new buffer is one line here.
  struct ScratchSet {
    Scratch level;     // second level of the moment reduction (long beams)
    Scratch tickets;   // ... and its per-sample tickets (k_reduce_moments_ticket, unsigned int): zero between launches
    Scratch obs;       // per-workgroup sums of x, y at the observers [B][chunks][2 * LYNX_MAX_OBSERVERS]
    Scratch erun;      // k_cavity_flags: every sample's energy on its way through the cavities
    Scratch esteps;    // k_cavity_flags_spec -> lanes build: every sample's energy behind 0, 1, ... step cavities [k][Bp]
    Scratch products;  // lanes = samples build: piece / pair products [slot][49][Bp] float64
    Scratch coefs;     // ... and cavity coefficients [S][8][Bp]
    Scratch steps[kTableSlots + 3];  // the ring of step tables, the reverse pass's own, the ParameterBeam lanes path's, the beam trace's
    Scratch trace[2];  // beam trace: the waves' slabs [B][waves][P][32] float64, the reference trajectory [B][P][8]
    Scratch trace_plan;  // ... with losses or screens: step codes and screen rows (TraceLosses.plan); lynx_ctx::trace_plan is what was uploaded last
    Scratch trace_jvp;  // lynx_track_*_along_forward: the directions (TraceDirections; lynx_ctx::trace_dirs is what was uploaded last), the entries' weight . dM [B][n][49] float64, a ParticleBeam's states mu [B][P][7], C [B][P][49] float64
    Scratch image_grad;  // lynx_gaussian_images_along_backward: the workgroups' partial sums [B][chunks][6] float64, screen after screen
    Scratch image_loss;  // lynx_gaussian_images_along_mse: the workgroups' partial sums [B][chunks][7] float64 of one screen, reused screen after screen
    Scratch units[2 * kTableSlots];  // compact unit records of multi-step float32 programs (lynx_units.hpp) and their class-D extras, per table slot
    Scratch units_bwd[2];  // ... and of the reverse pass's own table
    Scratch grad[3];   // backward: partials, T_bar, build scratch
    Scratch partials[kPartialRing];  // the workgroups' moment records, one buffer per slot of partial_ring
    Scratch* begin() { return reinterpret_cast<Scratch*>(this); }
    Scratch* end() { return reinterpret_cast<Scratch*>(this + 1); }
  } scratch;
  static_assert(std::is_standard_layout<Scratch>::value && sizeof(ScratchSet) % sizeof(Scratch) == 0, "ScratchSet: Scratch members only");
  int32_t* d_spec_valid = nullptr;   // whether scratch.esteps holds (k_cavity_flags)
  std::vector<int64_t> trace_plan;
  std::vector<int32_t> trace_dirs;   // the directions scratch.trace_jvp holds: dir_start | dir_leaf | dir_row | the weights' bits
  ncclComm_t comm = nullptr;
  int comm_ranks = 0;
  // The SIDE stream: what follows a streaming kernel without anything on this GPU waiting for it -- the reduction of
  // the workgroups' moment records and, with a communicator, the RCCL gather of the result -- runs here, underneath
  // the next call's streaming kernel, so that the main stream carries streaming kernels back to back.
  //   * a side operation starts behind the stop event that rides on its streaming kernel's dispatch (or a marker);
  //   * nothing on the main stream waits for it by itself: entry points that read moment records on the device
  //     join first (`join_side`), the host sees results through lynx_buf_d2h / lynx_sync, which wait for this stream;
  //   * the blocks it touches are kept out of the allocator until its "done" event has fired (`side_ops`);
  //   * the workgroups' records go through a ring of kPartialRing buffers; the host checks (and, rarely, waits)
  //     that a buffer's last reduction is done before a streaming kernel is given it again.
  hipStream_t s_side = nullptr;
  hipEvent_t ev_side_in = nullptr;    // side -> main (join_side)
  hipEvent_t ev_main_mark = nullptr;  // main -> side (a side operation whose input the main stream produces)
  struct SideOp {
    hipEvent_t done;
    const void* a;  // blocks the operation reads or writes (null: none)
    void* b;
    bool a_freed, b_freed;  // lynx_buf_free came while it was in flight: released when it is done
    bool owned;             // `done` goes back to side_events when the operation retires (else it belongs to a ring slot)
  };
  std::vector<SideOp> side_ops;         // in flight, oldest first (one stream: they finish in order)
  std::vector<hipEvent_t> side_events;  // idle "done" events
  bool side_busy = false;               // s_side may still be writing a block: readers wait for it
  bool level_on_side = false;           // which stream the users of scratch.level ran on last
  const void* side_wrote = nullptr;     // moment block the last side reduction writes (a gather of it needs no marker)
  struct PartialSlot {  // (its buffer: scratch.partials)
    hipEvent_t track_done = nullptr;  // rides on the streaming kernel's dispatch
    hipEvent_t reduced = nullptr;     // recorded on s_side behind the reduction
    bool pending = false;             // `reduced` has been recorded and not yet seen complete
  } partial_ring[kPartialRing];
  unsigned partial_seq = 0;
  // per-launch profiling of k_track (lynx_profile_begin / _end)
  bool profiling = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_events;
  std::vector<double> prof_ms;  // every launch of the last finished profile, in launch order
  std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_gather_events;  // ... and every RCCL gather (on the stream it ran on)
  std::vector<double> prof_gather_ms;
  hipEvent_t last_stream_stop = nullptr;
};

struct lynx_lattice {
  lynx_ctx* ctx = nullptr;
  int dtype = LYNX_F32;
  int64_t batch = 0;
  int32_t n_elems = 0, n_steps = 0;
  int32_t n_observers = 0;  // steps with LYNX_STEP_FLAG_OBSERVE (kept current by lynx_lattice_set_flags)
  bool has_cavity = false;  // any cavity element: its whole-batch predicates are evaluated on the device
  int32_t n_cavities = 0;
  int32_t* d_cav_words = nullptr;  // one word per cavity: the predicates OR-ed over the batch (k_cavity_flags_spec); kept zero between calls
  int2* d_cavs = nullptr;          // the cavities in lattice order: (element, its step if it is one of its own else -1)
  int32_t* d_cav_before = nullptr;  // [S + 1]: step cavities in front of step s (StepEnergies, lynx_device.hpp)
  int32_t n_step_cavities = 0;
  int64_t pool_count = 0;
  std::vector<lynx_elem> h_elems;
  std::vector<lynx_step> h_steps;
  lynx_elem* d_elems = nullptr;
  lynx_step* d_steps = nullptr;
  int32_t* d_elem_step = nullptr;
  void* d_pool = nullptr;
  // lanes = samples build (large batches): pieces, the levels of the pairwise tree over them, and
  // where each step's product ends up -- planned once from the step structure
  int plan_piece_len = 0;
  int32_t n_pieces = 0, n_slots = 0;
  std::vector<std::pair<int32_t, int32_t>> levels;  // (first task, number of tasks) per level
  BuildPiece* d_pieces = nullptr;
  PairTask* d_tasks = nullptr;
  int32_t* d_step_slot = nullptr;
  // multi-step float32 programs as units (lynx_units.hpp), one plan per value of `merged` (the forward and the reverse
  // pass may disagree about it, and a training loop that alternates between them must not re-plan every call):
  // whether it has been made since the flags last changed, whether the program fits it, and what k_emit_steps is told
  // about every step
  UnitPlan units[2];
  bool units_made[2] = {false, false};
  bool units_ok[2] = {false, false};
  int32_t* d_step_unit[2] = {nullptr, nullptr};
  // the reverse pass's (element, parameter) tasks, kind by kind (lynx_grad.hpp: bwd_kind_params), made on first use
  unsigned short* d_bwd_tasks = nullptr;
  int32_t n_bwd_tasks = 0;
  // Small lattices without cavities: the parameter pool travels by value in the arguments of the one-workgroup-per-
  // sample kernels (InlinePool, lynx_device.hpp).  A parameter write is a memcpy on the host; d_pool is brought up to
  // date when a kernel that reads it is next launched (sync_pool).
  uint64_t version = 0;  // parameter and flag writes so far
  bool prog_pool = false;
  bool pool_stale = false;
  InlinePool<kInlinePoolLarge> h_pool;
};

static thread_local std::string g_err;

static int fail(lynx_ctx* ctx, int code, const std::string& msg) {
  if (ctx) ctx->err = msg;
  g_err = msg;
  return code;
}

// the context (or lattice) an entry point is handed: NULL is an argument error, answered before anything touches it
#define LYNX_NEED(p)                                                                        \
  do {                                                                                      \
    if (!(p)) return fail(nullptr, LYNX_ERR_INVALID, "null " #p);                           \
  } while (0)

#define HIP_TRY(ctx, expr)                                                                  \
  do {                                                                                      \
    hipError_t _e = (expr);                                                                 \
    if (_e != hipSuccess)                                                                   \
      return fail((ctx), LYNX_ERR_HIP,                                                      \
                  std::string(#expr) + ": " + hipGetErrorString(_e) + " (" __FILE__ ":" +   \
                      std::to_string(__LINE__) + ")");                                      \
  } while (0)

#define NCCL_TRY(ctx, expr)                                                                 \
  do {                                                                                      \
    ncclResult_t _e = (expr);                                                               \
    if (_e != ncclSuccess)                                                                  \
      return fail((ctx), LYNX_ERR_RCCL, std::string(#expr) + ": " + ncclGetErrorString(_e)); \
  } while (0)

// The context's device as this thread's current one.  hipGetDevice reads a thread-local of the runtime; hipSetDevice,
// which every entry point used to call, takes the runtime's lock -- once per thread is enough.
static hipError_t use_device(lynx_ctx* ctx) {
  int current = -1;
  if (hipGetDevice(&current) == hipSuccess && current == ctx->device) return hipSuccess;
  return hipSetDevice(ctx->device);
}

// Events between the context's own streams, and the time stamps around a profiled launch, are recorded WITHOUT the
// system-scope fence HIP puts behind an event by default: that fence writes back and invalidates for the benefit of
// the host and of other devices, which nothing that waits on these events needs -- a kernel's own end-of-kernel release
// is what makes its results visible to the other queues of this device, host read-backs go through a copy and a stream
// synchronisation of their own, and RCCL fences what it sends.  Same box, alternating (scripts/gpu/r4/evscope.sh):
// BASELINE config 3 49.7-50.7 -> 47.0 us/step, the 128-sample shard of config 4 139.8-140.8 -> 135.8-136.2, config 3
// at 8 M particles 170.8-174.8 -> 168.5; hipEventReleaseToDevice instead: no change.
// With MORE THAN ONE RANK the events keep HIP's default: there a recorded event may also stand between RCCL's traffic from
// other devices and whoever reads it next, and none of that has run on hardware the builder had (lynx_ctx::plain_events).
static unsigned sync_event_flags(const lynx_ctx* ctx) {
  return hipEventDisableTiming | (ctx->plain_events ? 0u : (unsigned)hipEventDisableSystemFence);
}
static unsigned timing_event_flags(const lynx_ctx* ctx) {
  return hipEventDefault | (ctx->plain_events ? 0u : (unsigned)hipEventDisableSystemFence);
}

static hipError_t sync_main(lynx_ctx* ctx) {
  const hipError_t e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) ctx->main_idle = true;
  return e;
}

static size_t dtype_size(int dtype) { return dtype == LYNX_F64 ? 8 : 4; }

static size_t size_class(size_t bytes) {
  if (bytes == 0) bytes = 1;
  const size_t g = bytes >= (1u << 20) ? (1u << 20) : 256;
  return (bytes + g - 1) / g * g;
}

// Small result blocks the host reads right after the call (a sample's moment record: 288 bytes) can live in HOST memory
// the GPU writes through: reading them back then is a wait for the stream and a memcpy, not a copy command with a
// round trip of its own (BASELINE config 2 with sigma_x read after every call: NOTES.md).  Same allocator, another
// size-class name space (kHostVisible set in the class); `is_host_visible` tells lynx_buf_d2h and friends.
constexpr size_t kHostVisible = (size_t)1 << 62;
constexpr size_t kHostVisibleMax = 4096;

// caller holds ctx->mu
static void free_block(lynx_ctx* ctx, void* p, size_t size_class_key) {
  if (size_class_key & kHostVisible) {
    for (size_t i = 0; i < ctx->host_ranges.size(); ++i)
      if (ctx->host_ranges[i].first == (const char*)p) {
        ctx->host_ranges.erase(ctx->host_ranges.begin() + (long)i);
        break;
      }
    (void)hipHostFree(p);
  } else {
    (void)hipFree(p);
  }
}

static bool is_host_visible(lynx_ctx* ctx, const void* p) {
  std::lock_guard<std::mutex> lock(ctx->mu);
  for (const auto& r : ctx->host_ranges)
    if ((const char*)p >= r.first && (const char*)p < r.first + r.second) return true;
  return false;
}

static int ctx_alloc_host_visible(lynx_ctx* ctx, size_t bytes, void** out) {
  std::lock_guard<std::mutex> lock(ctx->mu);
  const size_t sc = size_class(bytes) | kHostVisible;
  auto it = ctx->free_blocks.find(sc);
  if (it != ctx->free_blocks.end()) {
    *out = it->second;
    ctx->free_blocks.erase(it);
    ctx->live[*out] = sc;
    return LYNX_OK;
  }
  void *p = nullptr, *d = nullptr;
  hipError_t e = hipHostMalloc(&p, sc & ~kHostVisible, hipHostMallocMapped | hipHostMallocCoherent);
  if (e == hipSuccess) e = hipHostGetDevicePointer(&d, p, 0);
  if (e != hipSuccess || d != p) {  // (one address for both sides is what the rest of the library assumes)
    if (p) (void)hipHostFree(p);
    (void)hipGetLastError();
    return fail(ctx, LYNX_ERR_NOMEM, std::string("hipHostMalloc (host-visible block): ") + hipGetErrorString(e));
  }
  ctx->live[p] = sc;
  ctx->host_ranges.emplace_back((const char*)p, sc & ~kHostVisible);
  *out = p;
  return LYNX_OK;
}

static int ctx_alloc(lynx_ctx* ctx, size_t bytes, void** out) {
  std::lock_guard<std::mutex> lock(ctx->mu);
  const size_t sc = size_class(bytes);
  auto it = ctx->free_blocks.find(sc);
  if (it != ctx->free_blocks.end()) {
    *out = it->second;
    ctx->free_blocks.erase(it);
    ctx->live[*out] = sc;
    return LYNX_OK;
  }
  void* p = nullptr;
  hipError_t e = hipMalloc(&p, sc);
  if (e != hipSuccess) {
    // give cached blocks back and retry once
    for (auto& kv : ctx->free_blocks) free_block(ctx, kv.second, kv.first);
    ctx->free_blocks.clear();
    e = hipMalloc(&p, sc);
    if (e != hipSuccess)
      return fail(ctx, LYNX_ERR_NOMEM, "hipMalloc(" + std::to_string(sc) + "): " + hipGetErrorString(e));
  }
  ctx->live[p] = sc;
  *out = p;
  return LYNX_OK;
}

// caller holds ctx->mu
static void release_block(lynx_ctx* ctx, void* p) {
  auto it = ctx->live.find(p);
  if (it == ctx->live.end()) return;
  ctx->free_blocks.emplace(it->second, p);
  ctx->live.erase(it);
}

// Side operations whose "done" event has fired leave the in-flight list (oldest first: s_side runs them in order);
// blocks that were freed meanwhile go back to the allocator now.  `wait`: block on every one of them.  Caller holds ctx->mu.
static void retire_side_ops(lynx_ctx* ctx, bool wait) {
  // a freed block goes back only with the LAST operation in flight that touches it (a reduction and the gather of
  // its result name the same block): an earlier one hands its mark on
  auto hand_on_or_release = [ctx](const void* p) {
    for (size_t k = 1; k < ctx->side_ops.size(); ++k) {
      lynx_ctx::SideOp& later = ctx->side_ops[k];
      if (later.a == p) { later.a_freed = true; return; }
      if (later.b == p) { later.b_freed = true; return; }
    }
    release_block(ctx, const_cast<void*>(p));
  };
  while (!ctx->side_ops.empty()) {
    lynx_ctx::SideOp& g = ctx->side_ops.front();
    if (wait) (void)hipEventSynchronize(g.done);
    else if (hipEventQuery(g.done) != hipSuccess) break;
    if (g.a_freed) hand_on_or_release(g.a);
    if (g.b_freed && g.b != g.a) hand_on_or_release(g.b);
    if (g.owned) ctx->side_events.push_back(g.done);
    ctx->side_ops.erase(ctx->side_ops.begin());
  }
}

static int ctx_free(lynx_ctx* ctx, void* p) {
  if (!p) return LYNX_OK;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (ctx->live.find(p) == ctx->live.end()) return fail(ctx, LYNX_ERR_INVALID, "lynx_buf_free: unknown pointer");
  if (!ctx->side_ops.empty()) {
    retire_side_ops(ctx, false);
    // a block an operation on the side stream still reads or writes: stream order on the main stream does not
    // protect it, so it stays out of the allocator until that operation is done
    bool held = false;
    for (auto& g : ctx->side_ops) {
      if (g.a == p) { g.a_freed = true; held = true; }
      if (g.b == p) { g.b_freed = true; held = true; }
    }
    if (held) return LYNX_OK;
  }
  release_block(ctx, p);
  return LYNX_OK;
}

static int ensure_scratch(lynx_ctx* ctx, Scratch& s, size_t need) {
  if (s.bytes >= need) return LYNX_OK;
  if (s.buf) {
    HIP_TRY(ctx, hipStreamSynchronize(ctx->s_build));
    HIP_TRY(ctx, sync_main(ctx));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->s_side));
    HIP_TRY(ctx, hipFree(s.buf));
    s = Scratch();
  }
  const size_t sz = size_class(need);
  HIP_TRY(ctx, hipMalloc(&s.buf, sz));
  s.bytes = sz;
  return LYNX_OK;
}

// per-sample tickets of k_reduce_moments_ticket, zeroed when they are (re)allocated; the kernel leaves them zero
static int ensure_tickets(lynx_ctx* ctx, size_t count) {
  Scratch& tickets = ctx->scratch.tickets;
  if (tickets.bytes >= count * sizeof(unsigned int)) return LYNX_OK;
  const int rc = ensure_scratch(ctx, tickets, std::max<size_t>(count, 1024) * sizeof(unsigned int));
  if (rc) return rc;
  // (hipMemset runs on the null stream and need not have finished when it returns; the context's streams do not wait for
  // that stream -- a reduction launched right behind this took tickets that the fill then wiped: one moment record of
  // zeros in the first call of a process, once in about thirty processes)
  HIP_TRY(ctx, hipMemsetAsync(tickets.buf, 0, tickets.bytes, ctx->stream));
  HIP_TRY(ctx, sync_main(ctx));
  return LYNX_OK;
}

// the GPU's compute units (256 if the runtime reports none)
static int64_t compute_units(const lynx_ctx* ctx) {
  return ctx->prop.multiProcessorCount > 0 ? ctx->prop.multiProcessorCount : 256;
}

// One body for both element types: `body` is a generic lambda that is handed a zero of the type -- `using T =
// decltype(zero);`.  Whatever is not LYNX_F64 is float (entry points that are handed a dtype and care check it themselves).
template <typename F>
static auto with_dtype(int dtype, F&& body) {
  return dtype == LYNX_F64 ? body(double()) : body(float());
}

// ---- the prologue of an entry point that enqueues on the main stream --------------------------
// Every such entry point reads, in this order:
//   LYNX_MAIN_ENTRY(ctx);                                    the context is there, and the main stream is idle no longer
//   ... its own checks (every refusal in front of what follows) ...
//   LYNX_MAIN_WRITES(ctx, kFeedsBuild | kFeedsNoBuild, {{pointer, bytes}, ...});
//                                                            this thread's device; what the call writes for the caller
// (lynx_track_particles and lynx_track_particles_backward say why they differ, where they do.)
#define LYNX_MAIN_ENTRY(ctx)                                                                \
  LYNX_NEED(ctx);                                                                           \
  (ctx)->main_idle = false /* (something is about to be enqueued on the main stream) */

// Device memory [p, p + bytes) that a call writes on the caller's behalf (a null pointer or no bytes: nothing).
struct Written {
  const void* p;
  size_t bytes;
};
// Whether the call's work on the main stream may write something that a later build on s_build reads -- its incoming
// energy or the lattice's parameter pool (BuildOrder::main_dirty has the rule).  kFeedsBuild: copies and fills between
// the caller's blocks, lynx_build_compose, the reverse passes, the ParameterBeam calls, the traces and the screen images
// along a trace, whose outputs a caller may hand to a track call as an energy.  kFeedsNoBuild: everything else -- an
// image, a mask, a moment record, a fresh beam, a diagnostic is never an energy or a pool, and a track call with steps
// says what it publishes itself (BuildOrder::streamed).
enum FeedsBuild : bool { kFeedsNoBuild = false, kFeedsBuild = true };

// what the call writes for the caller, without the device: for entry points that have never set it (lynx_buf_d2d,
// lynx_buf_memset) and for what is said behind a pass (lynx_track_particles_backward)
template <typename Outputs = std::initializer_list<Written>>
static void caller_blocks_written(lynx_ctx* ctx, FeedsBuild feeds, const Outputs& outputs) {
  for (const Written& w : outputs) ctx->wrote(w.p, w.bytes);
  if (feeds) ctx->order.main_wrote_build_input();
}

template <typename Outputs = std::initializer_list<Written>>
static int main_stream_writes(lynx_ctx* ctx, FeedsBuild feeds, const Outputs& outputs) {
  HIP_TRY(ctx, use_device(ctx));
  caller_blocks_written(ctx, feeds, outputs);
  return LYNX_OK;
}
#define LYNX_MAIN_WRITES(ctx, feeds, ...)                                                   \
  do {                                                                                      \
    if (const int rc_ = main_stream_writes((ctx), (feeds), __VA_ARGS__)) return rc_;        \
  } while (0)

// The API functions below get C linkage from their declarations in include/lynx_hip.h.

const char* lynx_version(void) { return "lynxhip 0.1.0 (gfx950)"; }

int lynx_device_count(int* count) {
  hipError_t e = hipGetDeviceCount(count);
  if (e != hipSuccess) {
    *count = 0;
    return fail(nullptr, LYNX_ERR_HIP, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
  }
  return LYNX_OK;
}

// the context's own inter-stream events (again, with other flags, when a communicator of more than one rank arrives)
static int make_sync_events(lynx_ctx* ctx) {
  const auto make = [&](hipEvent_t* e) -> hipError_t {
    if (*e) (void)hipEventDestroy(*e);
    *e = nullptr;
    return hipEventCreateWithFlags(e, sync_event_flags(ctx));
  };
  HIP_TRY(ctx, make(&ctx->ev_side_in));
  HIP_TRY(ctx, make(&ctx->ev_main_mark));
  for (auto& slot : ctx->partial_ring) {
    HIP_TRY(ctx, make(&slot.track_done));
    HIP_TRY(ctx, make(&slot.reduced));
    slot.pending = false;
  }
  for (int i = 0; i < lynx_ctx::kTableSlots; ++i) {
    HIP_TRY(ctx, make(&ctx->ev_built[i]));
    HIP_TRY(ctx, make(&ctx->order.ev_streamed_own[i]));
  }
  ctx->order.forget_stop_events();
  HIP_TRY(ctx, make(&ctx->order.ev_mark));
  for (hipEvent_t e : ctx->side_events) (void)hipEventDestroy(e);  // idle "done" events: made again on demand
  ctx->side_events.clear();
  return LYNX_OK;
}

int lynx_ctx_create(int device, lynx_ctx** out) {
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    return fail(nullptr, LYNX_ERR_HIP,
                std::string("no HIP device available: ") + (e != hipSuccess ? hipGetErrorString(e) : "count = 0"));
  if (device < 0 || device >= n) return fail(nullptr, LYNX_ERR_INVALID, "device ordinal out of range");
  lynx_ctx* ctx = new lynx_ctx();
  load_knobs(&ctx->knobs);
  ctx->device = device;
  HIP_TRY(nullptr, hipSetDevice(device));
  HIP_TRY(nullptr, hipGetDeviceProperties(&ctx->prop, device));
  HIP_TRY(nullptr, hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
  {
    // the build is short and the next streaming kernel waits for it: let its workgroups go first
    int prio_low = 0, prio_high = 0;
    HIP_TRY(nullptr, hipDeviceGetStreamPriorityRange(&prio_low, &prio_high));
    HIP_TRY(nullptr, hipStreamCreateWithPriority(&ctx->s_build, hipStreamNonBlocking, prio_high));
    HIP_TRY(nullptr, hipStreamCreateWithPriority(&ctx->s_side, hipStreamNonBlocking, prio_high));
  }
  {
    const char* world = getenv("WORLD_SIZE");  // (the launcher's; lynx_comm_init looks again)
    const char* plain = getenv("LYNX_PLAIN_EVENTS");  // (one rank's share of a job rehearsed in a process of its own)
    ctx->plain_events = (world && atoi(world) > 1) || (plain && atoi(plain) != 0);
    const int rc = make_sync_events(ctx);
    if (rc) return rc;
  }
  HIP_TRY(nullptr, hipEventCreate(&ctx->ev_start));
  HIP_TRY(nullptr, hipEventCreate(&ctx->ev_stop));
  HIP_TRY(nullptr, hipHostMalloc((void**)&ctx->h_status, 2 * sizeof(int32_t), hipHostMallocMapped));
  ctx->h_status[0] = ctx->h_status[1] = 0;
  HIP_TRY(nullptr, hipHostGetDevicePointer((void**)&ctx->d_status, ctx->h_status, 0));
  HIP_TRY(nullptr, hipMalloc((void**)&ctx->d_spec_valid, sizeof(int32_t)));
  HIP_TRY(nullptr, hipMemset(ctx->d_spec_valid, 0, sizeof(int32_t)));
  // the word hipStreamWaitValue32 polls: signal memory (what HIP documents for it); without it the build simply
  // starts at the head of the streaming kernel instead of in its tail
  if (hipDeviceGetAttribute(&ctx->can_wait_value, hipDeviceAttributeCanUseStreamWaitValue, device) != hipSuccess) ctx->can_wait_value = 0;
  if (ctx->can_wait_value &&
      hipExtMallocWithFlags((void**)&ctx->d_tail_flag, 8, hipMallocSignalMemory) != hipSuccess) {
    (void)hipGetLastError();
    ctx->d_tail_flag = nullptr;
    ctx->can_wait_value = 0;
  }
  if (ctx->d_tail_flag) HIP_TRY(nullptr, hipMemset(ctx->d_tail_flag, 0, 8));
  HIP_TRY(nullptr, hipDeviceSynchronize());  // (hipMemset runs on the null stream and need not have finished when it returns)
  *out = ctx;
  return LYNX_OK;
}

int lynx_ctx_destroy(lynx_ctx* ctx) {
  if (!ctx) return LYNX_OK;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->s_build);
  (void)sync_main(ctx);
  (void)hipStreamSynchronize(ctx->s_side);
  if (ctx->comm) (void)ncclCommDestroy(ctx->comm);
  {
    std::lock_guard<std::mutex> lock(ctx->mu);
    retire_side_ops(ctx, true);
  }
  for (auto* list : {&ctx->prof_events, &ctx->prof_gather_events})
    for (auto& pr : *list) {
      (void)hipEventDestroy(pr.first);
      (void)hipEventDestroy(pr.second);
    }
  (void)hipEventDestroy(ctx->ev_side_in);
  (void)hipEventDestroy(ctx->ev_main_mark);
  for (hipEvent_t e : ctx->side_events) (void)hipEventDestroy(e);
  for (auto& slot : ctx->partial_ring) {
    (void)hipEventDestroy(slot.track_done);
    (void)hipEventDestroy(slot.reduced);
  }
  (void)hipStreamDestroy(ctx->s_side);
  for (auto& kv : ctx->free_blocks) free_block(ctx, kv.second, kv.first);
  for (auto& kv : ctx->live) free_block(ctx, kv.first, kv.second);
  for (Scratch& s : ctx->scratch)
    if (s.buf) (void)hipFree(s.buf);
  if (ctx->d_spec_valid) (void)hipFree(ctx->d_spec_valid);
  for (int i = 0; i < lynx_ctx::kTableSlots; ++i) {
    (void)hipEventDestroy(ctx->ev_built[i]);
    (void)hipEventDestroy(ctx->order.ev_streamed_own[i]);
  }
  if (ctx->h_status) (void)hipHostFree(ctx->h_status);
  if (ctx->d_tail_flag) (void)hipFree(ctx->d_tail_flag);
  (void)hipEventDestroy(ctx->order.ev_mark);
  (void)hipEventDestroy(ctx->ev_start);
  (void)hipEventDestroy(ctx->ev_stop);
  (void)hipStreamDestroy(ctx->s_build);
  (void)hipStreamDestroy(ctx->stream);
  delete ctx;
  return LYNX_OK;
}

const char* lynx_last_error(lynx_ctx* ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

int lynx_device_info(lynx_ctx* ctx, lynx_device_info_t* out) {
  LYNX_NEED(ctx);
  memset(out, 0, sizeof(*out));
  snprintf(out->arch, sizeof(out->arch), "%s", ctx->prop.gcnArchName);
  // some driver stacks report no marketing name: the architecture then stands in for it
  if (ctx->prop.name[0]) snprintf(out->name, sizeof(out->name), "%s", ctx->prop.name);
  else snprintf(out->name, sizeof(out->name), "AMD GPU (%s)", ctx->prop.gcnArchName);
  out->compute_units = ctx->prop.multiProcessorCount;
  out->lds_bytes_per_cu = (int32_t)ctx->prop.maxSharedMemoryPerMultiProcessor;
  out->hbm_bytes = (int64_t)ctx->prop.totalGlobalMem;
  return LYNX_OK;
}

// s_side is the one stream whose work nothing on the main stream waits for by itself.
// Host readers (lynx_buf_d2h, lynx_sync): wait until it has drained.
static int wait_for_side(lynx_ctx* ctx) {
  if (ctx->side_busy) {
    HIP_TRY(ctx, hipStreamSynchronize(ctx->s_side));
    ctx->side_busy = false;
    std::lock_guard<std::mutex> lock(ctx->mu);
    retire_side_ops(ctx, true);
    for (auto& slot : ctx->partial_ring) slot.pending = false;
  }
  return LYNX_OK;
}

// a fresh or recycled "done" event for a side operation
static int side_event(lynx_ctx* ctx, hipEvent_t* out) {
  *out = nullptr;
  {
    std::lock_guard<std::mutex> lock(ctx->mu);
    retire_side_ops(ctx, false);
    // bounded backlog: the host blocks on the oldest operation rather than run arbitrarily far ahead
    while (ctx->side_ops.size() >= 32) {
      (void)hipEventSynchronize(ctx->side_ops.front().done);
      retire_side_ops(ctx, false);
    }
    if (!ctx->side_events.empty()) {
      *out = ctx->side_events.back();
      ctx->side_events.pop_back();
    }
  }
  if (!*out) HIP_TRY(ctx, hipEventCreateWithFlags(out, sync_event_flags(ctx)));
  return LYNX_OK;
}

// `done` has just been recorded on s_side behind an operation that touches blocks a and b
static void side_op_issued(lynx_ctx* ctx, hipEvent_t done, const void* a, void* b, bool owned = true) {
  std::lock_guard<std::mutex> lock(ctx->mu);
  ctx->side_ops.push_back(lynx_ctx::SideOp{done, a, b, false, false, owned});
  ctx->side_busy = true;
}

// What the kernels flagged since the last look; the caller has just waited for the GPU.
static int check_status(lynx_ctx* ctx) {
  if (ctx->h_status && __atomic_load_n(&ctx->h_status[0], __ATOMIC_ACQUIRE) != 0) {
    const int elem = __atomic_load_n(&ctx->h_status[1], __ATOMIC_ACQUIRE);
    __atomic_store_n(&ctx->h_status[0], 0, __ATOMIC_RELEASE);
    __atomic_store_n(&ctx->h_status[1], 0, __ATOMIC_RELEASE);
    return fail(ctx, LYNX_ERR_ENERGY,
                "Initial energy must be larger than 0 (a beam reached the cavity at element " + std::to_string(elem) +
                    " of its program with energy <= 0 or NaN; lynx/accelerator/cavity.py:260)");
  }
  return LYNX_OK;
}

// Device readers on the main stream (anything that may be handed a moment record or a gathered block): the main
// stream waits for what the side stream has been given so far.
static int join_side(lynx_ctx* ctx) {
  if (ctx->side_busy) {
    HIP_TRY(ctx, hipEventRecord(ctx->ev_side_in, ctx->s_side));
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_side_in, 0));
  }
  return LYNX_OK;
}

int lynx_sync(lynx_ctx* ctx) {
  LYNX_NEED(ctx);
  HIP_TRY(ctx, use_device(ctx));
  HIP_TRY(ctx, sync_main(ctx));
  const int rc = wait_for_side(ctx);
  return rc ? rc : check_status(ctx);
}

int lynx_timer_start(lynx_ctx* ctx) {
  LYNX_MAIN_ENTRY(ctx);
  HIP_TRY(ctx, hipEventRecord(ctx->ev_start, ctx->stream));
  return LYNX_OK;
}

int lynx_timer_stop(lynx_ctx* ctx, float* elapsed_ms) {
  LYNX_NEED(ctx);
  HIP_TRY(ctx, hipEventRecord(ctx->ev_stop, ctx->stream));
  HIP_TRY(ctx, hipEventSynchronize(ctx->ev_stop));
  ctx->main_idle = true;
  HIP_TRY(ctx, hipEventElapsedTime(elapsed_ms, ctx->ev_start, ctx->ev_stop));
  return LYNX_OK;
}

int lynx_profile_begin(lynx_ctx* ctx) {
  LYNX_NEED(ctx);
  // events of an earlier, unfinished profile may still stand in for step-table slots' "streamed" events: nothing may
  // wait on them once they are destroyed
  if (!ctx->prof_events.empty()) {
    HIP_TRY(ctx, hipStreamSynchronize(ctx->s_build));
    HIP_TRY(ctx, sync_main(ctx));
    ctx->order.forget_stop_events();
    ctx->last_stream_stop = nullptr;
  }
  for (auto& pr : ctx->prof_events) {
    (void)hipEventDestroy(pr.first);
    (void)hipEventDestroy(pr.second);
  }
  ctx->prof_events.clear();
  for (auto& pr : ctx->prof_gather_events) {
    (void)hipEventDestroy(pr.first);
    (void)hipEventDestroy(pr.second);
  }
  ctx->prof_gather_events.clear();
  ctx->profiling = true;
  return LYNX_OK;
}

int lynx_profile_end(lynx_ctx* ctx, double* total_ms, int64_t* launches) {
  LYNX_NEED(ctx);
  ctx->profiling = false;
  HIP_TRY(ctx, sync_main(ctx));
  // every build is followed by its streaming kernel on the main stream, so both streams are idle now;
  // the per-launch stop events stood in for the step-table slots' "streamed" events and go away here
  ctx->order.forget_stop_events();
  double total = 0.0;
  ctx->prof_ms.clear();
  for (auto& pr : ctx->prof_events) {
    float ms = 0.f;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, pr.first, pr.second));
    ctx->prof_ms.push_back(ms);
    total += ms;
    (void)hipEventDestroy(pr.first);
    (void)hipEventDestroy(pr.second);
  }
  *total_ms = total;
  *launches = (int64_t)ctx->prof_events.size();
  ctx->prof_events.clear();
  ctx->prof_gather_ms.clear();
  if (!ctx->prof_gather_events.empty()) {
    const int rc = wait_for_side(ctx);  // the gathers' stop events must have fired
    if (rc) return rc;
  }
  for (auto& pr : ctx->prof_gather_events) {
    float ms = 0.f;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, pr.first, pr.second));
    ctx->prof_gather_ms.push_back(ms);
    (void)hipEventDestroy(pr.first);
    (void)hipEventDestroy(pr.second);
  }
  ctx->prof_gather_events.clear();
  return LYNX_OK;
}

int lynx_profile_launches(lynx_ctx* ctx, double* ms_out, int64_t capacity, int64_t* launches) {
  if (!ctx || !launches || (capacity > 0 && !ms_out)) return fail(ctx, LYNX_ERR_INVALID, "null argument");
  *launches = (int64_t)ctx->prof_ms.size();
  for (int64_t i = 0; i < capacity && i < *launches; ++i) ms_out[i] = ctx->prof_ms[(size_t)i];
  return LYNX_OK;
}

int lynx_profile_gathers(lynx_ctx* ctx, double* ms_out, int64_t capacity, int64_t* gathers) {
  if (!ctx || !gathers || (capacity > 0 && !ms_out)) return fail(ctx, LYNX_ERR_INVALID, "null argument");
  *gathers = (int64_t)ctx->prof_gather_ms.size();
  for (int64_t i = 0; i < capacity && i < *gathers; ++i) ms_out[i] = ctx->prof_gather_ms[(size_t)i];
  return LYNX_OK;
}

int lynx_ctx_reload_knobs(lynx_ctx* ctx) {
  if (!ctx) return fail(ctx, LYNX_ERR_INVALID, "null argument");
  // plans made under the old settings (lanes-build pieces, unit plans) are keyed by what they depend on and are
  // re-made on demand; nothing in flight reads the knobs
  load_knobs(&ctx->knobs);
  return LYNX_OK;
}

int lynx_buf_alloc(lynx_ctx* ctx, size_t bytes, void** d_out) {
  LYNX_NEED(ctx);
  HIP_TRY(ctx, use_device(ctx));
  return ctx_alloc(ctx, bytes, d_out);
}

// A block for a RESULT the host is going to read back (a ParameterBeam's outgoing mu and cov, a moment record): small
// ones come from host memory the GPU writes through, so that lynx_buf_d2h is a wait and a memcpy (ctx_alloc_host_visible);
// large ones, and all of them once the context has a communicator, are device memory like any other block.
int lynx_buf_alloc_result(lynx_ctx* ctx, size_t bytes, void** d_out) {
  LYNX_NEED(ctx);
  HIP_TRY(ctx, use_device(ctx));
  if (bytes <= kHostVisibleMax && ctx->comm_ranks == 0 && ctx->knobs.host_visible_records) return ctx_alloc_host_visible(ctx, bytes, d_out);
  return ctx_alloc(ctx, bytes, d_out);
}

int lynx_buf_free(lynx_ctx* ctx, void* d_ptr) {
  if (ctx && d_ptr) ctx->wrote(d_ptr, 1);  // (a freed energy block may come back with other contents)
  return ctx_free(ctx, d_ptr);
}

int lynx_buf_h2d(lynx_ctx* ctx, void* d_dst, const void* h_src, size_t bytes) {
  LYNX_NEED(ctx);
  if (bytes == 0) return LYNX_OK;
  ctx->wrote(d_dst, bytes);
  if (is_host_visible(ctx, d_dst)) {  // host memory the GPU reads through: wait for whoever still uses it, then write
    const int rc = wait_for_side(ctx);
    if (rc) return rc;
    HIP_TRY(ctx, sync_main(ctx));
    memcpy(d_dst, h_src, bytes);
    return LYNX_OK;
  }
  HIP_TRY(ctx, hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, sync_main(ctx));  // h_src is pageable and may be freed
  return LYNX_OK;
}

int lynx_buf_d2h(lynx_ctx* ctx, void* h_dst, const void* d_src, size_t bytes) {
  LYNX_NEED(ctx);
  if (bytes == 0) return LYNX_OK;
  {
    const int rc = wait_for_side(ctx);  // the block may be a moment record or a gathered block
    if (rc) return rc;
  }
  if (is_host_visible(ctx, d_src)) {  // the GPU wrote it through to host memory: no copy command, just the wait
    HIP_TRY(ctx, sync_main(ctx));
    memcpy(h_dst, d_src, bytes);
    return check_status(ctx);
  }
  HIP_TRY(ctx, hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, sync_main(ctx));
  return check_status(ctx);  // what came back may be the result of a program that met a cavity with energy <= 0
}

int lynx_buf_d2d(lynx_ctx* ctx, void* d_dst, const void* d_src, size_t bytes) {
  LYNX_MAIN_ENTRY(ctx);
  if (bytes == 0) return LYNX_OK;
  {
    const int rc = join_side(ctx);  // the source may be a moment record the side stream is still reducing
    if (rc) return rc;
  }
  caller_blocks_written(ctx, kFeedsBuild, {{d_dst, bytes}});
  // (either side may be a host-visible block: the runtime works the direction out from the addresses)
  HIP_TRY(ctx, hipMemcpyAsync(d_dst, d_src, bytes, hipMemcpyDefault, ctx->stream));
  return LYNX_OK;
}

int lynx_buf_memset(lynx_ctx* ctx, void* d_dst, int value, size_t bytes) {
  LYNX_MAIN_ENTRY(ctx);
  if (bytes == 0) return LYNX_OK;
  {
    const int rc = join_side(ctx);
    if (rc) return rc;
  }
  caller_blocks_written(ctx, kFeedsBuild, {{d_dst, bytes}});
  HIP_TRY(ctx, hipMemsetAsync(d_dst, value, bytes, ctx->stream));
  return LYNX_OK;
}

int lynx_pool_trim(lynx_ctx* ctx) {
  LYNX_NEED(ctx);
  HIP_TRY(ctx, hipStreamSynchronize(ctx->s_build));
  HIP_TRY(ctx, sync_main(ctx));
  {
    const int rc = wait_for_side(ctx);
    if (rc) return rc;
  }
  std::lock_guard<std::mutex> lock(ctx->mu);
  for (auto& kv : ctx->free_blocks) free_block(ctx, kv.second, kv.first);
  ctx->free_blocks.clear();
  return LYNX_OK;
}

// ---- lattice ---------------------------------------------------------------------------

// observers must be single-identity-element run steps, at most LYNX_MAX_OBSERVERS of them
static int count_observers(lynx_ctx* ctx, lynx_lattice* lat) {
  int32_t n = 0;
  for (int32_t s = 0; s < lat->n_steps; ++s) {
    const lynx_step& st = lat->h_steps[s];
    if (!(st.flags & LYNX_STEP_FLAG_OBSERVE)) continue;
    if (st.kind != LYNX_STEP_RUN || st.last != st.first + 1 || lat->h_elems[st.first].kind != LYNX_KIND_IDENTITY)
      return fail(ctx, LYNX_ERR_INVALID, "an observer step must be a run of exactly one identity element");
    ++n;
  }
  if (n > LYNX_MAX_OBSERVERS) return fail(ctx, LYNX_ERR_INVALID, "too many observer steps in one program");
  lat->n_observers = n;
  return LYNX_OK;
}

static int params_of_kind(int kind) {
  switch (kind) {
    case LYNX_KIND_IDENTITY: return 0;
    case LYNX_KIND_DRIFT: return 1;
    case LYNX_KIND_QUADRUPOLE: return 5;
    case LYNX_KIND_DIPOLE: return 8;
    case LYNX_KIND_HCOR:
    case LYNX_KIND_VCOR: return 2;
    case LYNX_KIND_CAVITY: return 4;
    case LYNX_KIND_CUSTOM: return 49;
    case LYNX_KIND_BASE_RMATRIX: return 4;
    case LYNX_KIND_ROTATION: return 1;
    case LYNX_KIND_MISALIGNMENT: return 3;
    case LYNX_KIND_SOLENOID: return 4;
    case LYNX_KIND_UNDULATOR: return 1;
    default: return -1;
  }
}

// d_pool as current as the pool that travels in the kernel arguments: before any kernel that reads the parameters from memory
static int sync_pool(lynx_ctx* ctx, lynx_lattice* lat) {
  if (!lat->pool_stale) return LYNX_OK;
  HIP_TRY(ctx, hipMemcpyAsync(lat->d_pool, lat->h_pool.q, (size_t)lat->pool_count * dtype_size(lat->dtype), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, sync_main(ctx));
  lat->pool_stale = false;
  return LYNX_OK;
}

int lynx_lattice_create(lynx_ctx* ctx, int dtype, int64_t batch, int32_t n_elems,
                        const lynx_elem* elems, int32_t n_steps, const lynx_step* steps,
                        const void* pool, int64_t pool_count, lynx_lattice** out) {
  LYNX_NEED(ctx);
  *out = nullptr;
  if (dtype != LYNX_F32 && dtype != LYNX_F64) return fail(ctx, LYNX_ERR_INVALID, "bad dtype");
  if (batch <= 0 || n_elems < 0 || n_steps < 0 || pool_count < 0)
    return fail(ctx, LYNX_ERR_INVALID, "bad lattice sizes");
  // Validate every index the kernels will dereference: a bad table must never reach the GPU.
  std::vector<int32_t> elem_step(n_elems, -1);
  for (int32_t e = 0; e < n_elems; ++e) {
    const int np = params_of_kind(elems[e].kind);
    if (np < 0) return fail(ctx, LYNX_ERR_INVALID, "element " + std::to_string(e) + ": unknown kind");
    const int64_t bs = elems[e].batch_stride;
    if (bs != 0 && bs < np) return fail(ctx, LYNX_ERR_INVALID, "element batch_stride smaller than its row");
    const int64_t lo = elems[e].param_offset;
    const int64_t hi = lo + (batch - 1) * bs + np;
    if (lo < 0 || hi > pool_count)
      return fail(ctx, LYNX_ERR_INVALID, "element " + std::to_string(e) + ": parameters outside the pool");
  }
  int32_t next = 0;
  for (int32_t s = 0; s < n_steps; ++s) {
    const lynx_step& st = steps[s];
    if (st.first != next || st.last <= st.first || st.last > n_elems)
      return fail(ctx, LYNX_ERR_INVALID, "steps must tile the element list in order");
    if (st.kind == LYNX_STEP_CAVITY) {
      if (st.last != st.first + 1 || elems[st.first].kind != LYNX_KIND_CAVITY)
        return fail(ctx, LYNX_ERR_INVALID, "cavity step must hold exactly one cavity element");
    } else if (st.kind != LYNX_STEP_RUN) {
      return fail(ctx, LYNX_ERR_INVALID, "unknown step kind");
    }
    for (int32_t e = st.first; e < st.last; ++e) elem_step[e] = s;
    next = st.last;
  }
  if (next != n_elems) return fail(ctx, LYNX_ERR_INVALID, "steps do not cover every element");

  HIP_TRY(ctx, use_device(ctx));
  lynx_lattice* lat = new lynx_lattice();
  lat->ctx = ctx;
  lat->dtype = dtype;
  lat->batch = batch;
  lat->n_elems = n_elems;
  lat->n_steps = n_steps;
  lat->pool_count = pool_count;
  lat->h_elems.assign(elems, elems + n_elems);
  lat->h_steps.assign(steps, steps + n_steps);
  for (int32_t e = 0; e < n_elems; ++e) lat->n_cavities += elems[e].kind == LYNX_KIND_CAVITY ? 1 : 0;
  lat->has_cavity = lat->n_cavities > 0;
  const size_t es = dtype_size(dtype);
  int rc;
  if ((rc = count_observers(ctx, lat))) {
    delete lat;
    return rc;
  }
  if ((rc = ctx_alloc(ctx, std::max<size_t>(1, n_elems) * sizeof(lynx_elem), (void**)&lat->d_elems)) ||
      (rc = ctx_alloc(ctx, std::max<size_t>(1, n_steps) * sizeof(lynx_step), (void**)&lat->d_steps)) ||
      (rc = ctx_alloc(ctx, std::max<size_t>(1, n_elems) * sizeof(int32_t), (void**)&lat->d_elem_step)) ||
      (rc = ctx_alloc(ctx, std::max<size_t>(1, pool_count) * es, &lat->d_pool))) {
    delete lat;
    return rc;
  }
  HIP_TRY(ctx, hipMemcpyAsync(lat->d_elems, elems, n_elems * sizeof(lynx_elem), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(lat->d_steps, steps, n_steps * sizeof(lynx_step), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(lat->d_elem_step, elem_step.data(), n_elems * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(lat->d_pool, pool, pool_count * es, hipMemcpyHostToDevice, ctx->stream));
  if (lat->has_cavity) {
    if ((rc = ctx_alloc(ctx, (size_t)lat->n_cavities * sizeof(int32_t), (void**)&lat->d_cav_words))) {
      delete lat;
      return rc;
    }
    HIP_TRY(ctx, hipMemsetAsync(lat->d_cav_words, 0, (size_t)lat->n_cavities * sizeof(int32_t), ctx->stream));
    std::vector<int2> cavs;
    for (int32_t e = 0; e < n_elems; ++e)
      if (elems[e].kind == LYNX_KIND_CAVITY) cavs.push_back(make_int2(e, steps[elem_step[e]].kind == LYNX_STEP_CAVITY ? elem_step[e] : -1));
    if ((rc = ctx_alloc(ctx, cavs.size() * sizeof(int2), (void**)&lat->d_cavs))) {
      delete lat;
      return rc;
    }
    HIP_TRY(ctx, hipMemcpyAsync(lat->d_cavs, cavs.data(), cavs.size() * sizeof(int2), hipMemcpyHostToDevice, ctx->stream));
    std::vector<int32_t> before((size_t)n_steps + 1, 0);
    for (int32_t s = 0; s < n_steps; ++s) before[s + 1] = before[s] + (steps[s].kind == LYNX_STEP_CAVITY ? 1 : 0);
    lat->n_step_cavities = before[n_steps];
    if ((rc = ctx_alloc(ctx, before.size() * sizeof(int32_t), (void**)&lat->d_cav_before))) {
      delete lat;
      return rc;
    }
    HIP_TRY(ctx, hipMemcpyAsync(lat->d_cav_before, before.data(), before.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, sync_main(ctx));  // `cavs` and `before` go out of scope
  }
  HIP_TRY(ctx, sync_main(ctx));
  memset(&lat->h_pool, 0, sizeof(lat->h_pool));
  lat->prog_pool = !lat->has_cavity && n_steps > 0 && (size_t)pool_count * es <= sizeof(lat->h_pool);  // (a cavity's predicates are evaluated by kernels of their own)
  if (lat->prog_pool) memcpy(lat->h_pool.q, pool, (size_t)pool_count * es);
  *out = lat;
  return LYNX_OK;
}

int lynx_lattice_update_params(lynx_lattice* lat, int64_t offset, int64_t count, const void* host) {
  LYNX_NEED(lat);
  lynx_ctx* ctx = lat->ctx;
  if (offset < 0 || count < 0 || offset + count > lat->pool_count)
    return fail(ctx, LYNX_ERR_INVALID, "lynx_lattice_update_params: range outside the pool");
  const size_t es = dtype_size(lat->dtype);
  ++lat->version;
  if (lat->prog_pool) {  // the kernels of a small lattice read the parameters in their arguments: d_pool follows when it is needed
    memcpy(reinterpret_cast<unsigned char*>(lat->h_pool.q) + offset * es, host, count * es);
    lat->pool_stale = true;
    return LYNX_OK;
  }
  HIP_TRY(ctx, hipMemcpyAsync((char*)lat->d_pool + offset * es, host, count * es, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, sync_main(ctx));
  return LYNX_OK;
}

int lynx_lattice_set_flags(lynx_lattice* lat, const int32_t* elem_flags, const int32_t* step_flags) {
  LYNX_NEED(lat);
  lynx_ctx* ctx = lat->ctx;
  for (int32_t e = 0; e < lat->n_elems; ++e) lat->h_elems[e].flags = elem_flags[e];
  for (int32_t s = 0; s < lat->n_steps; ++s) lat->h_steps[s].flags = step_flags[s];
  lat->units_made[0] = lat->units_made[1] = false;  // the proposed classes depend on the elements' flags
  ++lat->version;
  {
    const int rc = count_observers(ctx, lat);
    if (rc) return rc;
  }
  HIP_TRY(ctx, hipMemcpyAsync(lat->d_elems, lat->h_elems.data(), lat->n_elems * sizeof(lynx_elem), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(lat->d_steps, lat->h_steps.data(), lat->n_steps * sizeof(lynx_step), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, sync_main(ctx));
  return LYNX_OK;
}

int lynx_lattice_destroy(lynx_lattice* lat) {
  if (!lat) return LYNX_OK;
  lynx_ctx* ctx = lat->ctx;
  {
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (ctx->fwd_table.lat == lat) ctx->fwd_table.valid = false;  // (the next lattice may get this address)
  }
  ctx_free(ctx, lat->d_elems);
  ctx_free(ctx, lat->d_steps);
  ctx_free(ctx, lat->d_elem_step);
  ctx_free(ctx, lat->d_pool);
  if (lat->d_cav_words) ctx_free(ctx, lat->d_cav_words);
  if (lat->d_cavs) ctx_free(ctx, lat->d_cavs);
  if (lat->d_cav_before) ctx_free(ctx, lat->d_cav_before);
  for (int32_t* p : lat->d_step_unit)
    if (p) ctx_free(ctx, p);
  if (lat->d_bwd_tasks) ctx_free(ctx, lat->d_bwd_tasks);
  if (lat->d_pieces) ctx_free(ctx, lat->d_pieces);
  if (lat->d_tasks) ctx_free(ctx, lat->d_tasks);
  if (lat->d_step_slot) ctx_free(ctx, lat->d_step_slot);
  delete lat;
  return LYNX_OK;
}

static LatticeDev dev_view(const lynx_lattice* lat) {
  LatticeDev d;
  d.elems = lat->d_elems;
  d.steps = lat->d_steps;
  d.elem_step = lat->d_elem_step;
  d.pool = lat->d_pool;
  d.batch = lat->batch;
  d.n_elems = lat->n_elems;
  d.n_steps = lat->n_steps;
  return d;
}

template <typename K>
static int allow_lds(lynx_ctx* ctx, K kernel, size_t bytes) {
  if (bytes > 160 * 1024)
    return fail(ctx, LYNX_ERR_INVALID,
                "program needs " + std::to_string(bytes) + " B of LDS (> 160 KiB): split the lattice");
  if (bytes > 48 * 1024)
    HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  return LYNX_OK;
}

// ---- build + compose -------------------------------------------------------------------

// Launch shape of k_build: 256 threads; chunks of <= 64 elements (<= 32 for float32 lattices, whose staging area
// would otherwise halve the resident workgroups) when the batch fills the GPU, of <= 128 when it does not -- then the
// tree depth is what a call waits for.  (Round 2 gave such a build 1024 threads; measured alone on one sample's
// 128-element float64 FODO, scripts/gpu/experiments/build_phases.hip: 1024 threads 18.0 us, 512: 13.1, 256: 11.3,
// 128: 13.6 -- sixteen waves of eight busy lanes each fetch the builders' code sixteen times and take 8.4 us for the
// first quadrupole where four waves of 32 take 4.6.)
// The long chunk needs ~90-115 KB of LDS: such a workgroup cannot be placed on a CU before a streaming kernel's
// workgroups there have drained, so a build that runs underneath the previous call's streaming kernel (`underneath`)
// keeps the short one (128-sample shard of BASELINE config 4: 18 us alone either way, 117-150 us with the long chunk vs
// the short chunk's share of the GPU under the streaming kernel).
// Returns the chunk.  `short_float32`: the limit of 32 is k_build's; the ParameterBeam kernels never took it.
template <typename T>
static int build_shape(lynx_ctx* ctx, const lynx_lattice* lat, bool underneath, bool short_float32) {
  const int64_t cus = compute_units(ctx);
  const bool deep = lat->batch * 2 <= cus && !underneath;
  // (float32, at most one workgroup per CU: 64 again -- half the rounds; the 128-sample shard of BASELINE config 4
  // underneath its streaming kernel: 0.1573 -> 0.1543 ms/step, medians of four, same box)
  const int limit = deep ? 128 : ((short_float32 && sizeof(T) == 4 && lat->batch > cus) ? 32 : 64);
  return build_chunk(lat->n_elems, limit);
}

// (a program of many steps: its table takes most of the LDS, and shorter chunks -- more compose rounds -- leave it room)
template <typename T>
static int fit_build_chunk(int chunk, const lynx_lattice* lat, size_t tail_scalars) {
  while (build_lds_layout(chunk, (size_t)lat->n_steps, sizeof(T), tail_scalars).total > (size_t)160 * 1024 && chunk > 8) chunk = (chunk + 1) / 2;
  return chunk;
}

// Where a workgroup kernel reads the lattice's parameters from: `launch()` for d_pool in memory, `launch(pool)` for the pool
// in the kernel's arguments -- its first 256 bytes when that is all of it, or all 1024 (lynx_device.hpp: InlinePool).
template <typename T, typename F>
static int with_pool_form(const lynx_lattice* lat, bool pool_in_args, F&& launch) {
  if (!pool_in_args) return launch();
  if ((size_t)lat->pool_count * sizeof(T) <= (size_t)kInlinePoolSmall)
    return launch(*reinterpret_cast<const InlinePool<kInlinePoolSmall>*>(&lat->h_pool));
  return launch(lat->h_pool);
}
// The kernel of each family that goes with a pool form
template <typename T> static auto build_kernel() { return k_build<T>; }
template <typename T, int BYTES> static auto build_kernel(const InlinePool<BYTES>&) { return k_build_inline<T, BYTES>; }
template <typename T> static auto track_moments_kernel() { return k_track_moments<T>; }
template <typename T, int BYTES> static auto track_moments_kernel(const InlinePool<BYTES>&) { return k_track_moments_inline<T, BYTES>; }
template <typename T> static auto build_bwd_kernel() { return k_build_bwd<T>; }
template <typename T, int BYTES> static auto build_bwd_kernel(const InlinePool<BYTES>&) { return k_build_bwd_inline<T, BYTES>; }

// Whole-batch cavity predicates for this call's energies, on `stream`, in front of whatever builds maps
// there (no-op for lattices without cavities).
template <typename T>
static int launch_cavity_flags(lynx_ctx* ctx, lynx_lattice* lat, hipStream_t stream, const void* d_energy_in,
                               bool for_lanes_build = false) {
  if (!lat->has_cavity || lat->n_steps == 0) return LYNX_OK;
  int rc;
  if ((rc = ensure_scratch(ctx, ctx->scratch.erun, (size_t)lat->batch * sizeof(T)))) return rc;
  // the lanes build reads every sample's energy in front of every step from what the first kernel computes on its way
  const int64_t Bp = (lat->batch + 63) / 64 * 64;
  T* e_steps = nullptr;
  if (for_lanes_build) {
    if ((rc = ensure_scratch(ctx, ctx->scratch.esteps, (size_t)(lat->n_step_cavities + 1) * Bp * sizeof(T)))) return rc;
    e_steps = (T*)ctx->scratch.esteps.buf;
  }
  // the predicates for every cavity at once, assuming every batch gains energy (one lane per sample), then one small
  // workgroup that checks the assumption, publishes the bits and -- should it not hold -- walks the serial way
  hipLaunchKernelGGL(k_cavity_flags_spec<T>, dim3((unsigned)((lat->batch + 255) / 256)), dim3(256), 0, stream, dev_view(lat),
                     lat->d_cavs, lat->n_cavities, (const T*)d_energy_in, lat->d_cav_words, e_steps, Bp);
  HIP_TRY(ctx, hipGetLastError());
  hipLaunchKernelGGL(k_cavity_flags<T>, dim3(1), dim3(256), 0, stream, dev_view(lat), lat->d_elems, lat->d_steps,
                     (const T*)d_energy_in, (T*)ctx->scratch.erun.buf, ctx->d_status, lat->d_cavs, lat->n_cavities,
                     lat->d_cav_words, e_steps ? ctx->d_spec_valid : (int32_t*)nullptr);
  HIP_TRY(ctx, hipGetLastError());
  return LYNX_OK;
}

// Plan of the lanes = samples build for this lattice: pieces of <= L elements inside each step, then
// levels of pair products until every step is one slot.
static int plan_lanes_build(lynx_ctx* ctx, lynx_lattice* lat, int L) {
  if (lat->plan_piece_len == L && lat->d_pieces) return LYNX_OK;
  std::vector<BuildPiece> pieces;
  std::vector<std::vector<int32_t>> live(lat->n_steps);
  for (int32_t s = 0; s < lat->n_steps; ++s) {
    const lynx_step& st = lat->h_steps[s];
    for (int32_t e = st.first; e < st.last; e += L) {
      live[s].push_back((int32_t)pieces.size());
      pieces.push_back(BuildPiece{e, std::min<int32_t>(e + L, st.last), s, 0});
    }
  }
  int32_t next = (int32_t)pieces.size();
  std::vector<PairTask> tasks;
  std::vector<std::pair<int32_t, int32_t>> levels;
  for (;;) {
    const int32_t first = (int32_t)tasks.size();
    for (auto& slots : live) {
      if (slots.size() < 2) continue;
      std::vector<int32_t> merged;
      for (size_t k = 0; k + 1 < slots.size(); k += 2) {
        tasks.push_back(PairTask{slots[k], slots[k + 1], next, 0});
        merged.push_back(next++);
      }
      if (slots.size() & 1) merged.push_back(slots.back());
      slots.swap(merged);
    }
    if ((int32_t)tasks.size() == first) break;
    levels.emplace_back(first, (int32_t)tasks.size() - first);
  }
  std::vector<int32_t> step_slot(std::max<int32_t>(1, lat->n_steps), 0);
  for (int32_t s = 0; s < lat->n_steps; ++s) step_slot[s] = live[s][0];
  if (lat->d_pieces) ctx_free(ctx, lat->d_pieces);
  if (lat->d_tasks) ctx_free(ctx, lat->d_tasks);
  if (lat->d_step_slot) ctx_free(ctx, lat->d_step_slot);
  lat->d_pieces = nullptr; lat->d_tasks = nullptr; lat->d_step_slot = nullptr;
  int rc;
  if ((rc = ctx_alloc(ctx, std::max<size_t>(1, pieces.size()) * sizeof(BuildPiece), (void**)&lat->d_pieces)) ||
      (rc = ctx_alloc(ctx, std::max<size_t>(1, tasks.size()) * sizeof(PairTask), (void**)&lat->d_tasks)) ||
      (rc = ctx_alloc(ctx, step_slot.size() * sizeof(int32_t), (void**)&lat->d_step_slot)))
    return rc;
  // copies on the main stream and a wait for them (planning happens once per lattice structure): the blocks come from
  // the caching allocator and a kernel on the context's streams -- which do not synchronise with the null stream -- may
  // still be reading what they held before
  HIP_TRY(ctx, hipMemcpyAsync(lat->d_pieces, pieces.data(), pieces.size() * sizeof(BuildPiece), hipMemcpyHostToDevice, ctx->stream));
  if (!tasks.empty())
    HIP_TRY(ctx, hipMemcpyAsync(lat->d_tasks, tasks.data(), tasks.size() * sizeof(PairTask), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(lat->d_step_slot, step_slot.data(), step_slot.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, sync_main(ctx));  // (the host vectors go out of scope)
  lat->plan_piece_len = L;
  lat->n_pieces = (int32_t)pieces.size();
  lat->n_slots = next;
  lat->levels.swap(levels);
  return LYNX_OK;
}

template <typename T>
static int launch_build_lanes(lynx_ctx* ctx, lynx_lattice* lat, hipStream_t stream, const void* d_energy_in,
                              void* d_steps_out, void* d_energy_out, int merge_pairs, float* d_units = nullptr,
                              float* d_extras = nullptr) {
  int rc;
  if ((rc = plan_lanes_build(ctx, lat, std::max(1, ctx->knobs.piece)))) return rc;
  const int64_t groups = (lat->batch + 63) / 64, Bp = groups * 64;
  if (lat->n_pieces > 65535 || lat->n_steps > 65535) return fail(ctx, LYNX_ERR_INVALID, "lattice too long for the lanes build");
  if ((rc = ensure_scratch(ctx, ctx->scratch.products, (size_t)lat->n_slots * 49 * Bp * sizeof(double))))
    return rc;
  if ((rc = ensure_scratch(ctx, ctx->scratch.coefs, (size_t)std::max(1, lat->n_steps) * 8 * Bp * sizeof(T))))
    return rc;
  const LatticeDev lv = dev_view(lat);
  const StepEnergies<T> se{lat->has_cavity ? (const T*)ctx->scratch.esteps.buf : (const T*)nullptr, lat->d_cav_before, ctx->d_spec_valid, Bp};
  if ((rc = allow_lds(ctx, k_build_pieces<T>, build_pieces_lds<T>()))) return rc;
  hipLaunchKernelGGL(k_build_pieces<T>, dim3((unsigned)groups, (unsigned)lat->n_pieces), dim3(64), build_pieces_lds<T>(), stream, lv,
                     lat->d_pieces, (const T*)d_energy_in, Bp, (double*)ctx->scratch.products.buf, (T*)ctx->scratch.coefs.buf, se);
  HIP_TRY(ctx, hipGetLastError());
  // narrow trees (BASELINE config 4: 8, 4, 2, 1 tasks per level) in one launch: underneath a streaming kernel every
  // launch of the chain costs ~20 us, the product itself 3-6 (config 4: 0.995 -> 0.985 ms/step, same box)
  bool narrow = !lat->levels.empty() && (int)lat->levels.size() <= kPairLevelsMax && ctx->knobs.pair_levels_fused != 0;
  for (const auto& level : lat->levels) narrow = narrow && level.second <= kPairLevelsMaxTasks;
  if (narrow) {
    PairLevels lv{};
    lv.n = (int32_t)lat->levels.size();
    for (int l = 0; l < lv.n; ++l) {
      lv.first[l] = lat->levels[l].first;
      lv.count[l] = lat->levels[l].second;
    }
    hipLaunchKernelGGL(k_pair_levels, dim3((unsigned)groups), dim3(256), 0, stream, lv, lat->d_tasks, lat->batch, Bp,
                       (double*)ctx->scratch.products.buf);
    HIP_TRY(ctx, hipGetLastError());
  } else {
    for (const auto& level : lat->levels) {
      hipLaunchKernelGGL(k_pair_products, dim3((unsigned)groups, (unsigned)level.second), dim3(64), 0, stream,
                         lat->d_tasks + level.first, lat->batch, Bp, (double*)ctx->scratch.products.buf);
      HIP_TRY(ctx, hipGetLastError());
    }
  }
  hipLaunchKernelGGL(k_emit_steps<T>, dim3((unsigned)groups, (unsigned)lat->n_steps), dim3(64), emit_steps_lds<T>(), stream, lv,
                     lat->d_step_slot, (const T*)d_energy_in, Bp, (const double*)ctx->scratch.products.buf,
                     (const T*)ctx->scratch.coefs.buf, merge_pairs, (T*)d_steps_out, (T*)d_energy_out,
                     d_units ? lat->d_step_unit[merge_pairs ? 1 : 0] : (const int32_t*)nullptr,
                     lat->units[merge_pairs ? 1 : 0].n_units, d_units, d_extras, se);
  HIP_TRY(ctx, hipGetLastError());
  return LYNX_OK;
}

// The unit records of a float32 step table that k_emit_steps did not write, behind the table's writer on `stream`
static int launch_pack_units(lynx_ctx* ctx, const lynx_lattice* lat, int merged, hipStream_t stream, const void* d_steps,
                             float* d_units, float* d_extras) {
  const UnitPlan& up = lat->units[merged ? 1 : 0];
  const int64_t n = lat->batch * up.n_units;
  hipLaunchKernelGGL(k_pack_units, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, up, lat->batch, lat->n_steps,
                     (const float*)d_steps, d_units, d_extras);
  HIP_TRY(ctx, hipGetLastError());
  return LYNX_OK;
}

// `d_units` / `d_extras`: also pack the unit records of a multi-step float32 program (the lattice's unit plan for `merge_pairs` must have been made);
// the lanes build does it while it writes the table, the workgroup build with k_pack_units behind it
template <typename T>
static int launch_build(lynx_ctx* ctx, lynx_lattice* lat, hipStream_t stream, const void* d_energy_in,
                        void* d_steps_out, void* d_energy_out, int merge_pairs = 0, bool underneath = false,
                        float* d_units = nullptr, float* d_extras = nullptr, bool force_lanes = false) {
  // large batches: lanes = samples (an order of magnitude fewer wave-instructions); small ones: one
  // workgroup per sample, whose tree is shallower than a chain of launches
  // (`force_lanes`: the workgroup build keeps the whole table in LDS; a caller whose table would not fit says so)
  const bool lanes = lat->n_steps > 0 && (force_lanes || lat->batch >= ctx->knobs.lanes_build_min_batch);
  {
    const int rc = launch_cavity_flags<T>(ctx, lat, stream, d_energy_in, lanes);
    if (rc) return rc;
  }
  if (lanes) {
    const int rc = sync_pool(ctx, lat);
    return rc ? rc : launch_build_lanes<T>(ctx, lat, stream, d_energy_in, d_steps_out, d_energy_out, merge_pairs, d_units, d_extras);
  }
  const int chunk = fit_build_chunk<T>(build_shape<T>(ctx, lat, underneath, true), lat, 0);
  const size_t lds = build_lds_layout(chunk, (size_t)lat->n_steps, sizeof(T), 0).total;
  // (the cavity flags are in front of everything here, in launch_track_moments behind sync_pool and allow_lds: the orders
  // never meet -- a lattice whose pool travels in the arguments has no cavity -- and each launcher keeps its own)
  const auto launch = [&](const auto&... pool) -> int {
    const auto kernel = build_kernel<T>(pool...);
    if constexpr (sizeof...(pool) == 0)
      if (const int stale = sync_pool(ctx, lat)) return stale;
    if (const int refused = allow_lds(ctx, kernel, lds)) return refused;
    hipLaunchKernelGGL(kernel, dim3((unsigned)lat->batch), dim3(256), lds, stream, pool..., dev_view(lat), (const T*)d_energy_in,
                       (T*)d_steps_out, (T*)d_energy_out, chunk, merge_pairs);
    HIP_TRY(ctx, hipGetLastError());
    return LYNX_OK;
  };
  if (const int rc = with_pool_form<T>(lat, lat->prog_pool && ctx->knobs.inline_pool, launch)) return rc;
  if constexpr (sizeof(T) == 4)
    if (d_units) return launch_pack_units(ctx, lat, merge_pairs, stream, d_steps_out, d_units, d_extras);
  return LYNX_OK;
}

int lynx_build_compose(lynx_ctx* ctx, lynx_lattice* lat, const void* d_energy_in, void* d_steps_out,
                       void* d_energy_out) {
  LYNX_MAIN_ENTRY(ctx);
  if (!lat || !d_energy_in || !d_steps_out) return fail(ctx, LYNX_ERR_INVALID, "null argument");
  if (lat->batch > 0x7fffffffLL) return fail(ctx, LYNX_ERR_INVALID, "batch too large");
  const size_t es = dtype_size(lat->dtype);
  LYNX_MAIN_WRITES(ctx, kFeedsBuild, {{d_steps_out, (size_t)lat->batch * lat->n_steps * LYNX_STEP_STRIDE * es},
                                      {d_energy_out, (size_t)lat->batch * es}});
  return with_dtype(lat->dtype, [&](auto zero) {
    return launch_build<decltype(zero)>(ctx, lat, ctx->stream, d_energy_in, d_steps_out, d_energy_out);
  });
}

// ---- particle tracking -----------------------------------------------------------------

struct TrackPlan {
  hipEvent_t done = nullptr;  // recorded when the streaming kernel has finished (may be null)
  bool full_cov; // accumulate the whole covariance (21 products) instead of the property set (8)
  int unroll;    // particles per lane and iteration
  int mom_mode;  // 1 = float64 per particle, 2 = float32 partial sums per iteration, 3 = float32 lane sums
  bool xpose;    // wave tiles through LDS (full-width accesses) instead of per-particle accesses
  TrackArgs a;
  size_t lds;
  unsigned grid;
};

template <typename T>
static TrackPlan plan_track(lynx_ctx* ctx, const lynx_lattice* lat, int64_t B, int64_t N, int32_t S, bool moments,
                            bool full_cov) {
  TrackPlan p;
  p.full_cov = full_cov;
  constexpr int P = 16 / (int)sizeof(T);  // particles per lane of a wave tile
  const int64_t cus = compute_units(ctx);
  const Knobs& kn = ctx->knobs;
  const int64_t target = 512 * cus;  // workgroups per CU over the whole launch
  p.mom_mode = knob(kn.mom, sizeof(T) == 4 ? 2 : 1);
  if (sizeof(T) == 8 || p.mom_mode < 2 || p.mom_mode > 3) p.mom_mode = sizeof(T) == 4 ? 2 : 1;
  p.a.n_particles = N;
  p.a.store = 0;
  p.a.tail_flag = nullptr;
  p.a.tail_seq = 0;
  p.a.tail_wg = 0;
  p.a.stash_offset = 0;
  p.a.reversed = 0;
  // wave tiles: with non-temporal full-width stores +7 % on single-map float32 programs (BASELINE config 4:
  // 5.4 -> 5.8 TB/s) and +10 % (+7 % of that from the stores) on float64 (config 3 at 8 M particles); slower on
  // multi-step float32 programs, which want two particles per lane, not four
  // (a read-only pass -- lynx_moments, S = 0 -- has no stores to gain from and stays with per-particle loads)
  const bool single_map = S == 1 && lat && lat->h_steps[0].kind == LYNX_STEP_RUN &&
                          !(lat->h_steps[0].flags & LYNX_STEP_FLAG_OBSERVE);
  // (with the whole covariance in float32 lane sums the tile form runs out of registers: 1.23 vs 1.13 ms on C4)
  // (and short samples leave most wave tiles cut: 700 particles per sample 0.79 vs 0.72 ms per 20 M particles)
  p.xpose = knob(kn.xpose, ((sizeof(T) == 8 || (single_map && !full_cov)) && N >= 8 * 64 * P) ? 1 : 0) != 0;
  int u = knob(kn.unroll, p.xpose ? P : (sizeof(T) == 4 ? (S > 1 ? 2 : 4) : 1));
  if (u != 1 && u != 2 && u != 4) u = 2;
  if (sizeof(T) == 8 && u > 2) u = 2;
  // small jobs: fewer particles per lane so that more workgroups exist
  while (u > 1 && B * ((N + 256 * u - 1) / (256 * u)) < 4 * cus) u >>= 1;
  if (u != P) p.xpose = false;
  p.unroll = u;
  const int64_t tile = 256 * (int64_t)u;
  const int64_t ntiles = (N + tile - 1) / tile;
  // A workgroup pays a fixed cost (table load, 29-value cross-lane reduction, partial
  // record), so it gets at least `min_tpw` tiles -- unless that would leave CUs idle.
  // Measured with the round-2 kernels (property-set moments, scripts/gpu/r2_c4sweep.sh, same box): single-map
  // programs like many short-lived workgroups -- 2 tiles each: C4 5.26 -> 5.49 TB/s, c3big 4.83 -> 5.09 --
  // while multi-step programs also fetch S step records per iteration and want long-lived ones (C5 with
  // 2 / 4 / 8 / 16 tiles: 1.25 / 1.14 / 1.10 / 1.09 ms).
  int64_t min_tpw = std::max(1, knob(kn.min_tiles_per_wg, S > 1 ? 16 : 2));
  while (min_tpw > 1 && B * ((ntiles + min_tpw - 1) / min_tpw) < 4 * cus) --min_tpw;
  int64_t chunks = std::max<int64_t>(1, std::min<int64_t>((ntiles + min_tpw - 1) / min_tpw, (target + B - 1) / B));
  // A launch of a FEW rounds of workgroups is better off as ONE round of longer-lived ones: a workgroup of the single-map
  // kernels takes ~10 us whatever it does (table load, first tile's latency, moment epilogue), three of them fit a CU
  // (162-164 registers), and BASELINE config 3 as worded -- one sample, 1 M particles, 1954 tiles -- ran 1954 one-tile
  // workgroups in 2.5 rounds: 28.9 us; 652 workgroups of three tiles: 23.7 (46 -> 39 us a step).  Launches of many rounds
  // keep their short-lived workgroups (capped the same way: c3big 155 -> 189 us, config 4 0.96 -> 1.2-1.3 ms).
  {
    const int64_t one_round = 3 * cus;
    const int cap = knob(kn.one_round, (S <= 1 && B * chunks > one_round && B * chunks <= 4 * one_round) ? 3 : 0);
    if (cap > 0) chunks = std::max<int64_t>(1, std::min<int64_t>(chunks, cap * cus / B));
  }
  int64_t tpw = (ntiles + chunks - 1) / chunks;
  chunks = (ntiles + tpw - 1) / tpw;
  p.a.chunks = (int32_t)chunks;
  p.a.tiles_per_wg = (int32_t)tpw;
  // float32 lane sums for the whole workgroup are fine while a lane sees few particles
  if (p.mom_mode == 2 && kn.mom < 0 && tpw * u <= 32) p.mom_mode = 3;
  if (p.mom_mode == 3 && tpw * u > 64) p.mom_mode = 2;
  size_t scratch = 4 * kPartialStride * sizeof(double);
  if (moments)
    scratch = std::max<size_t>(scratch, (size_t)(full_cov ? kMomSlabScalars : kMomSlabScalarsCompact) * (p.mom_mode >= 2 ? 4 : 8));
  if (p.xpose) scratch = std::max<size_t>(scratch, (size_t)(kTrackThreads / 64) * kWaveTileBytes);
  scratch = (scratch + 15) / 16 * 16;
  p.a.lds_scratch_bytes = (int32_t)scratch;
  p.a.n_observers = lat ? lat->n_observers : 0;
  p.lds = track_lds_layout<T>(scratch, (size_t)S, (size_t)p.a.n_observers).total;
  p.grid = (unsigned)(B * chunks);
  return p;
}

// The launch of a streaming kernel, whichever it is: p.grid workgroups with `lds` bytes on the main stream.
template <typename K, typename... Args>
static int launch_streaming(lynx_ctx* ctx, const TrackPlan& p, K kernel, size_t lds, const Args&... args) {
  int rc = allow_lds(ctx, kernel, lds);
  if (rc) return rc;
  // Events ride on the dispatch itself (hipExtLaunchKernelGGL: start / stop timestamps of this kernel)
  // instead of separate marker packets in front of and behind it: `done` is what the build stream waits
  // for before it reuses the step-table slot, and with profiling on (bench.py) the pair is also the
  // kernel's duration.
  hipEvent_t e0 = nullptr, e1 = p.done;
  if (ctx->profiling) {  // every profiled launch needs time stamps of its own
    HIP_TRY(ctx, hipEventCreateWithFlags(&e0, timing_event_flags(ctx)));
    HIP_TRY(ctx, hipEventCreateWithFlags(&e1, timing_event_flags(ctx)));
  }
  hipExtLaunchKernelGGL(kernel, dim3(p.grid), dim3(kTrackThreads), (std::uint32_t)lds, ctx->stream, e0, e1, 0u, args...);
  HIP_TRY(ctx, hipGetLastError());
  if (ctx->profiling) ctx->prof_events.emplace_back(e0, e1);
  ctx->last_stream_stop = e1;  // what "this streaming kernel has finished" is, for the build stream
  return LYNX_OK;
}

// What a launch of k_track_direct is made of, whichever instantiation it takes.
struct DirectLaunch {
  lynx_ctx* ctx;
  const TrackPlan& p;
  const LatticeDev& lv;
  const void *d_energy_in, *d_p_in;
  void *d_p_out, *d_energy_out;
  const void* d_steps;
  double *d_partials, *d_obs;
};

template <typename T, int MOM, bool FULL, int UNROLL, bool XPOSE>
static int launch_direct_inst(const DirectLaunch& l) {
  return launch_streaming(l.ctx, l.p, k_track_direct<T, MOM, FULL, UNROLL, XPOSE>, l.p.lds, l.lv, l.p.a, (const T*)l.d_energy_in,
                          (const T*)l.d_p_in, (T*)l.d_p_out, (T*)l.d_energy_out, (const T*)l.d_steps, l.d_partials, l.d_obs);
}

template <typename T, int MOM, bool FULL, int U>
static int launch_direct_mu(const DirectLaunch& l) {
  if constexpr (U * 7 * sizeof(T) == 112) {
    if (l.p.xpose) return launch_direct_inst<T, MOM, FULL, U, true>(l);
  }
  return launch_direct_inst<T, MOM, FULL, U, false>(l);
}

template <typename T, int MOM, bool FULL>
static int launch_direct_m(const DirectLaunch& l) {
  switch (l.p.unroll) {
    case 1: return launch_direct_mu<T, MOM, FULL, 1>(l);
    case 2: return launch_direct_mu<T, MOM, FULL, 2>(l);
    default:
      if constexpr (sizeof(T) == 4) return launch_direct_mu<T, MOM, FULL, 4>(l);
      else return fail(l.ctx, LYNX_ERR_INVALID, "float64: at most 2 particles per lane");
  }
}

template <typename T>
static int launch_direct(const DirectLaunch& l, bool moments) {
  const int mom = moments ? l.p.mom_mode : 0;
  if (mom == 0) return launch_direct_m<T, 0, false>(l);
  if constexpr (sizeof(T) == 4) {
    if (mom == 3) return l.p.full_cov ? launch_direct_m<T, 3, true>(l) : launch_direct_m<T, 3, false>(l);
    return l.p.full_cov ? launch_direct_m<T, 2, true>(l) : launch_direct_m<T, 2, false>(l);
  } else {
    return l.p.full_cov ? launch_direct_m<T, 1, true>(l) : launch_direct_m<T, 1, false>(l);
  }
}

// ---- multi-step float32 programs as units (lynx_units.hpp) ------------------------------------

// Class a unit's map is expected to have, from the kinds and whole-batch flags of its elements (the numbers are checked
// per sample by k_pack_units; a wrong guess costs speed, never correctness).
static int proposed_class(const lynx_lattice* lat, int32_t first, int32_t last) {
  int rank = 1;  // 1 = U, 2 = D, 3 = dense
  for (int32_t e = first; e < last; ++e) {
    const lynx_elem& el = lat->h_elems[e];
    switch (el.kind) {
      case LYNX_KIND_IDENTITY:
      case LYNX_KIND_DRIFT:
      case LYNX_KIND_HCOR:
      case LYNX_KIND_VCOR:
      case LYNX_KIND_CAVITY:
      case LYNX_KIND_UNDULATOR: break;
      case LYNX_KIND_QUADRUPOLE: rank = std::max(rank, (el.flags & LYNX_FLAG_TILT) ? 3 : 1); break;
      case LYNX_KIND_DIPOLE: rank = std::max(rank, 2); break;  // a tilted one fails the numeric check
      default: rank = 3; break;                                // solenoid, custom map, helper kinds
    }
  }
  return rank == 1 ? kClassU : rank == 2 ? kClassD : kClassDense;
}

// The program as units: a step, or (merged) a run together with the active cavity behind it.  False if it does not fit.
static bool plan_units(const lynx_lattice* lat, bool merged, UnitPlan* plan) {
  const int32_t S = lat->n_steps;
  plan->n_units = 0;
  for (int32_t s = 0; s < S; ++s) {
    const lynx_step& st = lat->h_steps[s];
    if (st.flags & LYNX_STEP_FLAG_OBSERVE) return false;
    const bool pair = merged && s + 1 < S && st.kind == LYNX_STEP_RUN && lat->h_steps[s + 1].kind == LYNX_STEP_CAVITY;
    const int32_t last = pair ? lat->h_steps[s + 1].last : st.last;
    if (pair) ++s;
    if (plan->n_units >= kMaxUnits || s > 255) return false;
    const int u = plan->n_units++;
    plan->slot[u] = (unsigned char)s;
    plan->pair[u] = pair ? 1 : 0;
    plan->cls[u] = (unsigned char)proposed_class(lat, st.first, last);
  }
  for (int u = plan->n_units; u < kMaxUnits; ++u) plan->slot[u] = plan->cls[u] = plan->pair[u] = 0;
  return plan->n_units > 0;
}

// The lattice's unit plan for `merged`, made once per lattice and flag change; with it the table k_emit_steps reads.
static int ensure_units_plan(lynx_ctx* ctx, lynx_lattice* lat, bool merged) {
  const int m = merged ? 1 : 0;
  if (lat->units_made[m]) return LYNX_OK;
  UnitPlan& up = lat->units[m];
  lat->units_ok[m] = plan_units(lat, merged, &up) && lat->batch * up.n_units * kUnitStride < 0x7fffffffLL;
  lat->units_made[m] = true;
  if (!lat->units_ok[m]) return LYNX_OK;
  std::vector<int32_t> code((size_t)lat->n_steps, -1);
  for (int u = 0; u < up.n_units; ++u) code[up.slot[u]] = step_unit_code(u, up.cls[u], up.pair[u]);
  int rc;
  if (!lat->d_step_unit[m] && (rc = ctx_alloc(ctx, code.size() * sizeof(int32_t), (void**)&lat->d_step_unit[m]))) return rc;
  // rare (new lattice, or its flags changed): nothing may still be reading the old table
  HIP_TRY(ctx, hipStreamSynchronize(ctx->s_build));
  HIP_TRY(ctx, sync_main(ctx));
  HIP_TRY(ctx, hipMemcpy(lat->d_step_unit[m], code.data(), code.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  return LYNX_OK;
}

// What a launch of the unit kernels is made of, whichever instantiation it takes.
struct UnitsLaunch {
  lynx_ctx* ctx;
  const TrackPlan& p;
  int32_t U, S;
  const void* d_p_in;
  void *d_p_out, *d_energy_out;
  const void *d_steps, *d_units, *d_extras;
  double* d_partials;
};

template <int MOM, bool FULL, int PAIRS, bool PAIR_FORM = false>
static int launch_units_inst(const UnitsLaunch& l) {
  const size_t lds = units_lds_bytes((size_t)l.p.a.lds_scratch_bytes, l.U);
  auto kernel = k_track_units<MOM, FULL, PAIRS>;
  if constexpr (PAIR_FORM) kernel = k_track_unit_pairs<MOM, FULL>;
  return launch_streaming(l.ctx, l.p, kernel, lds, l.p.a, l.U, l.S, (const float*)l.d_p_in, (float*)l.d_p_out, (float*)l.d_energy_out,
                          (const float*)l.d_steps, (const float*)l.d_units, (const float*)l.d_extras, l.d_partials);
}

static int launch_units(const UnitsLaunch& l, bool moments, bool pair_form) {
  const TrackPlan& p = l.p;
  // every unit proposed as a merged [run, cavity] pair of class U: k_track_unit_pairs
  if (pair_form) return moments ? launch_units_inst<3, false, 1, true>(l) : launch_units_inst<0, false, 1, true>(l);
  if (p.unroll == 4) {  // two pairs per lane
    if (!moments) return launch_units_inst<0, false, 2>(l);
    if (p.mom_mode == 3) return p.full_cov ? launch_units_inst<3, true, 2>(l) : launch_units_inst<3, false, 2>(l);
    return p.full_cov ? launch_units_inst<2, true, 2>(l) : launch_units_inst<2, false, 2>(l);
  }
  if (!moments) return launch_units_inst<0, false, 1>(l);
  if (p.mom_mode == 3) return p.full_cov ? launch_units_inst<3, true, 1>(l) : launch_units_inst<3, false, 1>(l);
  return p.full_cov ? launch_units_inst<2, true, 1>(l) : launch_units_inst<2, false, 1>(l);
}

// The step table of one track call (S > 0): the slot of the ring it took, how it was built, and what the streaming kernel
// reads of it.
struct TrackTable {
  int slot = -1;            // of the ring of tables (-1: S = 0, no table)
  bool async = false;       // built on the second stream
  bool tail = false;        // ... behind the tail of an earlier streaming kernel: this call's kernel announces its own
  bool short_call = false;  // from half a million particles up to 128 MB of them, no cavity
  const void* d_steps = nullptr;
  float* d_units = nullptr;  // use_units: the slot's compact unit records and their class-D extras
  float* d_extras = nullptr;
  int n_units = 0;
  bool use_units = false;   // the structured step loop (k_track_units / k_track_unit_pairs) walks this call
};

// -- the stages of track_table --

// The merged form: [run, cavity] pairs as one unit for the packed float32 step loop (one 7x7 application per pair;
// LYNX_TRACK_SEQUENTIAL_STEPS keeps every step on its own), and with it the LDS stash behind the table.
template <typename T>
static void table_merged_form(const lynx_ctx* ctx, const lynx_lattice* lat, int32_t S, int flags, TrackPlan& p) {
  bool has_pair = false;
  for (int32_t s = 1; s < S; ++s)
    has_pair |= lat->h_steps[s].kind == LYNX_STEP_CAVITY && lat->h_steps[s - 1].kind == LYNX_STEP_RUN &&
                !(lat->h_steps[s - 1].flags & LYNX_STEP_FLAG_OBSERVE);
  p.a.merged_pairs = has_pair && sizeof(T) == 4 && p.unroll == 2 &&
                     !(flags & LYNX_TRACK_SEQUENTIAL_STEPS) && ctx->knobs.merge_steps;
  if (p.a.merged_pairs) {  // four floats of LDS per lane for pairs that take the rows form (kEntryStash)
    const TrackLds l = track_lds_layout<T>((size_t)p.a.lds_scratch_bytes, (size_t)S, (size_t)p.a.n_observers);
    p.a.stash_offset = (int32_t)l.stash;
    p.lds = l.stash + l.stash_bytes;
  }
}

// Where the build runs (t->short_call, t->async).
// The second stream pays once the streaming kernel is long enough to hide a build under; below half a
// million particles per call the extra event traffic costs more host time than the overlap returns
// (BASELINE config 2: 31 -> 46 us per call with it).
// SHORT calls in between (from half a million particles up to 128 MB of them: BASELINE config 3, 1 M particles,
// 29 us of kernel) take what the queue says: kernels of one queue follow each other without a gap, a hop to
// another queue costs 10-20 us of latency (kernel timeline, profiles/r04_*_timeline.txt).  If the main stream is
// IDLE -- the caller waits for every result -- there is nothing to hide the build under and the hops are pure
// loss: build, stream and reduce back to back on the main stream, no event at all.  If it is BUSY -- calls are
// pipelined -- the build goes to the second stream, where it runs underneath the previous call's kernels, and only
// the reduction stays in line (the side stream's hop is worth it for long kernels only).
template <typename T>
static void table_build_stream(const lynx_ctx* ctx, const lynx_lattice* lat, int64_t B, int64_t N, TrackTable* t) {
  const bool half_million = B * N >= (int64_t)512 << 10;
  t->short_call = half_million && (size_t)B * N * 7 * sizeof(T) < ((size_t)128 << 20) && !lat->has_cavity;
  bool inline_all = false;
  if (t->short_call && ctx->knobs.async_build < 0)
    inline_all = knob(ctx->knobs.small_inline, ctx->main_idle ? 1 : 0) != 0;
  t->async = knob(ctx->knobs.async_build, half_million && !inline_all ? 1 : 0) != 0;
}

// An asynchronous build behind what it reads (BuildOrder::order_build), and whether it starts in a tail (t->tail).
static int table_order_build(lynx_ctx* ctx, const void* d_energy_in, TrackTable* t) {
  t->tail = ctx->can_wait_value && ctx->knobs.build_in_tail && !t->short_call;  // (a short kernel has no tail worth waiting for)
  const bool wait_for_tail = t->tail && ctx->tail_seq >= 2;
  HIP_TRY(ctx, ctx->order.order_build(ctx->s_build, ctx->stream, t->slot, d_energy_in, wait_for_tail ? ctx->d_tail_flag : nullptr,
                                      ctx->tail_seq - 1));
  return LYNX_OK;
}

// The structured step loop: whether this call takes it (t->use_units), and room for its records in the table's slot.
// Multi-step float32 programs are walked as units with structured maps (lynx_units.hpp); LYNX_TRACK_UNITS=0 keeps the
// dense step loop of k_track_direct (LYNX_TRACK_UNITS=2: insist -- an error if this call cannot take the structured
// loop; for tests).
template <typename T>
static int table_unit_records(lynx_ctx* ctx, lynx_lattice* lat, int64_t B, int64_t N, int32_t S, const TrackPlan& p, TrackTable* t) {
  if constexpr (sizeof(T) == 4) {
    int rc;
    const int want_units = ctx->knobs.track_units;
    const int m = p.a.merged_pairs ? 1 : 0;
    // (k_track_units addresses a sample's particles with 32-bit byte offsets: samples below 4 GiB)
    if (S > 1 && (p.unroll == 2 || p.unroll == 4) && !p.xpose && p.a.n_observers == 0 && want_units &&
        (uint64_t)N * 28u + ((uint64_t)1 << 20) < ((uint64_t)1 << 32)) {
      if ((rc = ensure_units_plan(ctx, lat, p.a.merged_pairs != 0))) return rc;
      t->use_units = lat->units_ok[m];
    }
    if (want_units == 2 && !t->use_units)
      return fail(ctx, LYNX_ERR_INVALID, "LYNX_TRACK_UNITS=2: this call does not take the structured step loop");
    if (t->use_units) {
      const int64_t n = B * lat->units[m].n_units;
      Scratch &units = ctx->scratch.units[t->slot], &extras = ctx->scratch.units[lynx_ctx::kTableSlots + t->slot];
      if ((rc = ensure_scratch(ctx, units, (size_t)n * kUnitStride * sizeof(float))) ||
          (rc = ensure_scratch(ctx, extras, (size_t)n * kUnitExtraStride * sizeof(float))))
        return rc;
      t->d_units = (float*)units.buf;
      t->d_extras = (float*)extras.buf;
      t->n_units = lat->units[m].n_units;
    }
  }
  return LYNX_OK;
}

// The build's launch on its stream, and who waits for an asynchronous one.
template <typename T>
static int table_launch_build(lynx_ctx* ctx, lynx_lattice* lat, int64_t B, int64_t N, const void* d_energy_in, const TrackPlan& p,
                              TrackTable* t) {
  int rc;
  hipStream_t bs = t->async ? ctx->s_build : ctx->stream;
  if ((rc = launch_build<T>(ctx, lat, bs, d_energy_in, ctx->scratch.steps[t->slot].buf, nullptr, p.a.merged_pairs, t->async, t->d_units,
                            t->d_extras)))
    return rc;
  t->d_steps = ctx->scratch.steps[t->slot].buf;
  if (!t->async) return LYNX_OK;
  HIP_TRY(ctx, hipEventRecord(ctx->ev_built[t->slot], bs));
  // The HOST waits for the build instead of the main stream: no barrier packet with a foreign signal in front of
  // the streaming kernel (measured on the 128-sample shard of BASELINE config 4: step - kernel 18.8 -> 8.5-10 us,
  // c3big 17.9 -> 8-14, config 4 itself 20 -> 14).  The build of this call started when the streaming kernel of
  // call n - kTableSlots + 1 began, so by now the GPU still has about two calls queued.  Not for lattices with
  // cavities: their build (k_cavity_flags + the lanes kernels) takes most of a streaming kernel's time next to a
  // VALU-bound kernel, and the host's wake-up would sit on the critical path (BASELINE config 5: 0.932 -> 0.947
  // ms/step with it).  LYNX_BUILD_HOST_WAIT=0 / 1 forces the main-stream / host wait.
  // Nor for short streaming kernels (BASELINE config 3, 1 M particles: 29 us of kernel, 22 us of build -- the
  // host would be the pacemaker: 48 -> 75 us/step): from 128 MB of particles per call.
  const bool long_kernel = (size_t)B * N * 7 * sizeof(T) >= ((size_t)128 << 20);
  if (knob(ctx->knobs.build_host_wait, (lat->has_cavity || !long_kernel) ? 0 : 1)) HIP_TRY(ctx, hipEventSynchronize(ctx->ev_built[t->slot]));
  else HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_built[t->slot], 0));
  return LYNX_OK;
}

// Builds the step table of this call: takes the next slot of the ring, then stage by stage -- the merged form
// (p.a.merged_pairs and the LDS stash), where the build runs, what it waits for, the structured step loop's records, the
// launch and who waits for it -- and leaves the table to a reverse pass that may follow (lynx_ctx::fwd_table).
template <typename T>
static int track_table(lynx_ctx* ctx, lynx_lattice* lat, int64_t B, int64_t N, int32_t S, const void* d_energy_in,
                       const void* d_energy_out, int flags, TrackPlan& p, TrackTable* t) {
  int rc;
  t->slot = (int)(ctx->seq++ % (unsigned)lynx_ctx::kTableSlots);
  if ((rc = ensure_scratch(ctx, ctx->scratch.steps[t->slot], (size_t)B * S * LYNX_STEP_STRIDE * sizeof(T)))) return rc;
  table_merged_form<T>(ctx, lat, S, flags, p);
  table_build_stream<T>(ctx, lat, B, N, t);
  if (t->async && (rc = table_order_build(ctx, d_energy_in, t))) return rc;
  if ((rc = table_unit_records<T>(ctx, lat, B, N, S, p, t))) return rc;
  if ((rc = table_launch_build<T>(ctx, lat, B, N, d_energy_in, p, t))) return rc;
  std::lock_guard<std::mutex> lock(ctx->mu);
  ctx->fwd_table.leave(lat, lat->version, d_energy_in, (size_t)B * sizeof(T), d_energy_out, t->slot, p.a.merged_pairs, t->use_units,
                       ctx->seq);
  return LYNX_OK;
}

// Records of the workgroups (`rows` per sample, in the ring slot's buffer) -> record of the sample, on the side stream
// behind the streaming kernel's stop event (`side`) or in line on the main stream.  One 256-thread workgroup per sample
// walks up to 70 rows; more rows go through a level of <= 64 groups first (rows_per_group grows with the beam).
static int reduce_moment_records(lynx_ctx* ctx, int64_t B, int rows, bool side, lynx_ctx::PartialSlot* ring,
                                 const double* d_partials, double* d_moments_out) {
  int rc;
  hipStream_t rs = ctx->stream;
  if (side) {
    rs = ctx->s_side;
    HIP_TRY(ctx, hipStreamWaitEvent(rs, ctx->last_stream_stop, 0));
  } else {
    // in line: the side stream may still be reducing into a block the allocator has not seen freed; the main
    // stream's own order covers everything else
    ctx->side_wrote = nullptr;
  }
  const double* level_in = d_partials;
  constexpr size_t lds = reduce_lds_bytes<256, kReduceStage>();
  if (rows > kReduceStage) {
    const int rpg = std::max((rows + 63) / 64, B <= 4 ? 32 : 1);  // (few samples: no point in groups of a handful of rows)
    const int groups = (rows + rpg - 1) / rpg;
    const size_t need = (size_t)B * groups * kPartialStride * sizeof(double);
    // one buffer: its users follow each other on one stream (side or main), and a change of stream joins first
    if ((rc = ensure_scratch(ctx, ctx->scratch.level, need))) return rc;
    if (ctx->level_on_side != side) {
      if (side) {  // earlier in-line levels ran on the main stream: the side stream waits for them
        HIP_TRY(ctx, hipEventRecord(ctx->ev_main_mark, ctx->stream));
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->s_side, ctx->ev_main_mark, 0));
      } else if ((rc = join_side(ctx))) {
        return rc;
      }
      ctx->level_on_side = side;
    }
    if (ctx->knobs.reduce_ticket) {
      // both levels in one launch: the workgroup that draws a sample's last ticket adds its group records up
      if ((rc = ensure_tickets(ctx, (size_t)B))) return rc;
      hipLaunchKernelGGL((k_reduce_moments_ticket<256, kReduceStage>), dim3((unsigned)(B * groups)), dim3(256), lds, rs,
                         level_in, rows, rpg, groups, (double*)ctx->scratch.level.buf, (unsigned int*)ctx->scratch.tickets.buf, d_moments_out);
      HIP_TRY(ctx, hipGetLastError());
      rows = 0;
    } else {
      hipLaunchKernelGGL((k_reduce_moments<false, 256, kReduceStage>), dim3((unsigned)(B * groups)), dim3(256), lds, rs,
                         level_in, rows, rpg, groups, (double*)ctx->scratch.level.buf);
      HIP_TRY(ctx, hipGetLastError());
      level_in = (const double*)ctx->scratch.level.buf;
      rows = groups;
    }
  }
  if (rows > 0) {
    hipLaunchKernelGGL((k_reduce_moments<true, 256, kReduceStage>), dim3((unsigned)B), dim3(256), lds, rs, level_in,
                       rows, rows, 1, d_moments_out);
    HIP_TRY(ctx, hipGetLastError());
  }
  if (side) {
    // one event: the ring slot's.  The host has seen its previous recording complete before this call took the
    // slot, so whatever side operation still carries it has finished and retires on the next look.
    {
      std::lock_guard<std::mutex> lock(ctx->mu);
      retire_side_ops(ctx, false);
    }
    HIP_TRY(ctx, hipEventRecord(ring->reduced, rs));
    ring->pending = true;
    side_op_issued(ctx, ring->reduced, d_moments_out, nullptr, false);
    ctx->side_wrote = d_moments_out;
  }
  return LYNX_OK;
}

// One track call: plan, step table, record buffers, streaming launch, moment reduction.
template <typename T>
static int track_particles_t(lynx_ctx* ctx, lynx_lattice* lat, const LatticeDev& lv, int64_t B, int64_t N,
                             const void* d_energy_in, const void* d_p_in, void* d_p_out, void* d_energy_out,
                             double* d_moments_out, int flags, double* d_observations = nullptr) {
  const int32_t S = lv.n_steps;
  const bool moments = (flags & (LYNX_TRACK_MOMENTS | LYNX_TRACK_COVARIANCE)) != 0;
  const bool full_cov = (flags & LYNX_TRACK_COVARIANCE) != 0;
  TrackPlan p = plan_track<T>(ctx, lat, B, N, S, moments, full_cov);
  p.a.store = d_p_out ? 1 : 0;
  const bool shared_in = (flags & LYNX_TRACK_SHARED_INPUT) != 0;
  p.a.in_stride = shared_in ? 0 : N * 7;
  p.a.merged_pairs = 0;
  int rc;
  // what this call writes for the caller may hold the incoming energy of the table kept for a reverse pass
  // (kFeedsNoBuild: a call with steps says what it publishes behind its launch, BuildOrder::streamed; the outgoing energy
  // of a program without steps is a copy on the main stream, below, that a later build may read: kFeedsBuild)
  caller_blocks_written(ctx, kFeedsNoBuild, {{d_p_out, (size_t)B * N * 7 * sizeof(T)},
                                             {d_moments_out, (size_t)B * LYNX_MOMENT_STRIDE * sizeof(double)},
                                             {d_observations, lat ? (size_t)B * lat->n_observers * 2 * sizeof(double) : 0}});
  caller_blocks_written(ctx, S == 0 ? kFeedsBuild : kFeedsNoBuild, {{d_energy_out, (size_t)B * sizeof(T)}});
  // The build is always a launch of its own (in the streaming kernel's prologue it measured the same twice: NOTES.md,
  // "Tried and dropped in round 4"), so a call with steps always takes a slot of the ring and leaves a FwdTable.
  TrackTable t;
  if (S > 0 && (rc = track_table<T>(ctx, lat, B, N, S, d_energy_in, d_energy_out, flags, p, &t))) return rc;
  // A program without steps has no table for the kernel to take the outgoing energy from: the beam leaves with the
  // energy it came in with, copied here on the main stream.
  if (S == 0 && d_energy_out && d_energy_out != d_energy_in) {
    HIP_TRY(ctx, hipMemcpyAsync(d_energy_out, d_energy_in, (size_t)B * sizeof(T), hipMemcpyDefault, ctx->stream));
  }
  if ((int64_t)B * p.a.chunks > 0x7fffffffLL) return fail(ctx, LYNX_ERR_INVALID, "grid too large");
  // Workgroup records: a ring of buffers, so that the reduction of call n (side stream) can still read its records
  // while the streaming kernels of calls n+1.. write theirs.  The host makes sure the slot's previous reduction is done.
  double* d_partials = nullptr;
  lynx_ctx::PartialSlot* ring = nullptr;
  // The reduction leaves the main stream once the streaming kernel is long enough to hide it under (same threshold
  // as the build's second stream: below it the extra event traffic costs more host time than it returns).
  const bool side = moments && knob(ctx->knobs.side_reduce, (B * N >= (int64_t)512 << 10 && !t.short_call) ? 1 : 0) != 0;
  if (moments) {
    const unsigned ring_slot = ctx->partial_seq++ % lynx_ctx::kPartialRing;
    ring = &ctx->partial_ring[ring_slot];
    if (ring->pending) {
      if (hipEventQuery(ring->reduced) != hipSuccess) HIP_TRY(ctx, hipEventSynchronize(ring->reduced));
      ring->pending = false;
    }
    const size_t need = (size_t)B * p.a.chunks * kPartialStride * sizeof(double);
    if ((rc = ensure_scratch(ctx, ctx->scratch.partials[ring_slot], need))) return rc;
    d_partials = (double*)ctx->scratch.partials[ring_slot].buf;
  }
  double* d_obs = nullptr;
  if (p.a.n_observers) {
    if (!d_observations) return fail(ctx, LYNX_ERR_INVALID, "the program has observer steps: d_observations required");
    const size_t need = (size_t)B * p.a.chunks * 2 * LYNX_MAX_OBSERVERS * sizeof(double);
    if ((rc = ensure_scratch(ctx, ctx->scratch.obs, need))) return rc;
    d_obs = (double*)ctx->scratch.obs.buf;
  }
  if (t.tail) {  // this kernel announces its tail: one of the workgroups of its last round of dispatches
    p.a.tail_flag = ctx->d_tail_flag;
    p.a.tail_seq = ++ctx->tail_seq;
    p.a.tail_wg = (int32_t)std::max<int64_t>(0, (int64_t)p.grid - 4 * compute_units(ctx));
  }
  // Every other LONG call walks the batch from its end: what the previous pass left in the 256 MB Infinity Cache -- the
  // end of its incoming beam -- is then what this one reads first, if it is the same beam again (the optimisation loop:
  // one incoming beam, new settings every step).  BASELINE config 3 at 8 M particles (448 MB in): 171 -> 161.5 us/step;
  // config 4 (2.87 GB in): 980.6 -> 972.  Same workgroups, same records, another order of dispatch.
  if (!t.use_units && ctx->knobs.alternate_order &&
      (ctx->knobs.alternate_order == 2 || (size_t)B * N * 7 * sizeof(T) >= ((size_t)256 << 20)))
    p.a.reversed = ctx->knobs.alternate_order == 2 ? 1 : (int32_t)(ctx->long_calls++ & 1u);
  // the time stamp on the dispatch is what a later build on the second stream waits for before it reuses the
  // table slot; a call whose build ran on the main stream leaves it out (BuildOrder::streamed)
  p.done = (t.slot >= 0 && t.async) ? ctx->order.stop_event(t.slot) : nullptr;
  if (side && !p.done) p.done = ring->track_done;  // the side stream's reduction starts behind it
  if (t.use_units) {
    const UnitPlan& up = lat->units[p.a.merged_pairs ? 1 : 0];
    bool pair_form = ctx->knobs.unit_pairs != 0;
    for (int u = 0; u < up.n_units && pair_form; ++u) pair_form = up.cls[u] == kClassU && up.pair[u];
    pair_form = pair_form && p.unroll != 4 && (!moments || (p.mom_mode == 3 && !p.full_cov));  // (the forms that fit 88 registers)
    if (ctx->knobs.unit_pairs == 2 && !pair_form)
      rc = fail(ctx, LYNX_ERR_INVALID, "LYNX_UNIT_PAIRS=2: this call does not take the kernel for lattices of [run, cavity] pairs");
    else
      rc = launch_units({ctx, p, t.n_units, S, d_p_in, d_p_out, d_energy_out, t.d_steps, t.d_units, t.d_extras, d_partials}, moments, pair_form);
  } else {
    rc = launch_direct<T>({ctx, p, lv, d_energy_in, d_p_in, d_p_out, d_energy_out, t.d_steps, d_partials, d_obs}, moments);
  }
  if (rc) {
    if (t.tail) --ctx->tail_seq;  // nothing will announce this number: a later build must not wait for it
    return rc;
  }
  if (p.a.n_observers) {
    hipLaunchKernelGGL(k_reduce_observers, dim3((unsigned)B), dim3(64), 0, ctx->stream, d_obs, p.a.chunks,
                       p.a.n_observers, (double)N, d_observations);
    HIP_TRY(ctx, hipGetLastError());
  }
  ctx->order.streamed(t.slot, t.async, ctx->last_stream_stop, d_energy_out);
  if (moments) return reduce_moment_records(ctx, B, p.a.chunks, side, ring, d_partials, d_moments_out);
  return LYNX_OK;
}

int lynx_track_particles(lynx_ctx* ctx, lynx_lattice* lat, int64_t n_particles, const void* d_energy_in,
                         const void* d_p_in, void* d_p_out, void* d_energy_out, double* d_moments_out,
                         int flags, double* d_observations) {
  if (!ctx || !lat || !d_p_in) return fail(ctx, LYNX_ERR_INVALID, "null argument");
  if (n_particles <= 0) return fail(ctx, LYNX_ERR_INVALID, "n_particles must be > 0");
  if ((lat->n_steps > 0 || d_energy_out) && !d_energy_in) return fail(ctx, LYNX_ERR_INVALID, "energy_in required");
  if ((flags & (LYNX_TRACK_MOMENTS | LYNX_TRACK_COVARIANCE)) && !d_moments_out)
    return fail(ctx, LYNX_ERR_INVALID, "LYNX_TRACK_MOMENTS / LYNX_TRACK_COVARIANCE need d_moments_out");
  if ((flags & LYNX_TRACK_SHARED_INPUT) && d_p_in == d_p_out)
    return fail(ctx, LYNX_ERR_INVALID, "a shared incoming beam cannot be tracked in place");
  HIP_TRY(ctx, use_device(ctx));
  LatticeDev lv = dev_view(lat);
  const int rc = with_dtype(lat->dtype, [&](auto zero) {
    return track_particles_t<decltype(zero)>(ctx, lat, lv, lat->batch, n_particles, d_energy_in, d_p_in, d_p_out, d_energy_out,
                                             d_moments_out, flags, d_observations);
  });
  ctx->main_idle = false;  // (whatever allocation inside may have waited for the stream: work follows it now)
  return rc;
}

int lynx_track_particles_new(lynx_ctx* ctx, lynx_lattice* lat, int64_t n_particles, const void* d_energy_in,
                             const void* d_p_in, int flags, int32_t want_energy_out, void** d_out /* [4] */) {
  if (!ctx || !lat || !d_out) return fail(ctx, LYNX_ERR_INVALID, "null argument");
  for (int k = 0; k < 4; ++k) d_out[k] = nullptr;
  if (n_particles <= 0) return fail(ctx, LYNX_ERR_INVALID, "n_particles must be > 0");
  const size_t es = dtype_size(lat->dtype);
  const bool moments = (flags & (LYNX_TRACK_MOMENTS | LYNX_TRACK_COVARIANCE)) != 0;
  int rc = ctx_alloc(ctx, (size_t)lat->batch * (size_t)n_particles * 7 * es, &d_out[0]);
  if (!rc && want_energy_out) rc = ctx_alloc(ctx, (size_t)lat->batch * es, &d_out[1]);
  if (!rc && moments) {
    // a few samples' records, one process: where the host reads them without a copy command (many samples, or records
    // that RCCL gathers: device memory)
    const size_t bytes = (size_t)lat->batch * LYNX_MOMENT_STRIDE * sizeof(double);
    if (bytes <= kHostVisibleMax && ctx->comm_ranks == 0 && ctx->knobs.host_visible_records) rc = ctx_alloc_host_visible(ctx, bytes, &d_out[2]);
    else rc = ctx_alloc(ctx, bytes, &d_out[2]);
  }
  if (!rc && lat->n_observers > 0) rc = ctx_alloc(ctx, (size_t)lat->batch * lat->n_observers * 2 * sizeof(double), &d_out[3]);
  if (!rc)
    rc = lynx_track_particles(ctx, lat, n_particles, d_energy_in, d_p_in, d_out[0], d_out[1], (double*)d_out[2], flags,
                              (double*)d_out[3]);
  if (rc) {  // nothing was enqueued on these blocks (every check of lynx_track_particles comes before its first launch ...
    const std::string why = ctx->err;
    (void)sync_main(ctx);  // ... but a failure halfway through a launch sequence may have: drain first)
    for (int k = 0; k < 4; ++k) {
      if (d_out[k]) (void)ctx_free(ctx, d_out[k]);
      d_out[k] = nullptr;
    }
    ctx->err = why;
  }
  return rc;
}

// ---- reverse pass -----------------------------------------------------------------------

// k_build_bwd's task list for this lattice: (element, parameter | energy) pairs kind by kind, every kind padded to whole
// waves of 64 (lynx_grad.hpp).  The kinds of a lattice never change: made once.
static int ensure_bwd_tasks(lynx_ctx* ctx, lynx_lattice* lat) {
  if (lat->d_bwd_tasks) return LYNX_OK;
  std::vector<unsigned short> tasks;
  if (lat->n_elems >= 4096) return fail(ctx, LYNX_ERR_INVALID, "reverse pass: at most 4095 elements per program");
  for (int k = 1; k <= LYNX_KIND_UNDULATOR; ++k) {
    const int np = bwd_kind_params(k);
    if (np == 0) continue;
    const size_t first = tasks.size();
    for (int32_t e = 0; e < lat->n_elems; ++e)
      if (lat->h_elems[e].kind == k)
        for (int q = 0; q <= np; ++q) tasks.push_back((unsigned short)(e * 16 + (q == np ? kGradParams : q)));
    if (tasks.size() > first)
      while (tasks.size() & 63) tasks.push_back(0xffffu);  // a wave never mixes kinds
  }
  if (tasks.empty()) tasks.assign(64, 0xffffu);
  int rc = ctx_alloc(ctx, tasks.size() * sizeof(unsigned short), (void**)&lat->d_bwd_tasks);
  if (rc) return rc;
  // on the main stream, not the null stream: the block may be one a kernel still in flight there was reading
  HIP_TRY(ctx, hipMemcpyAsync(lat->d_bwd_tasks, tasks.data(), tasks.size() * sizeof(unsigned short), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, sync_main(ctx));  // (the host vector goes out of scope)
  lat->n_bwd_tasks = (int32_t)tasks.size();
  return LYNX_OK;
}

constexpr int kBwdWgsPerCu = 24;                     // workgroups per CU of the reverse streaming kernels
constexpr size_t kBwdMapsLdsBytes = (size_t)40 << 10;  // k_build_bwd keeps maps and prefix products in LDS up to this

// What every reverse pass ends with.  A sweep leaves T_bar [B][S][kGradStride] in scratch.grad[1]; k_build_bwd, with its
// maps and prefix products in scratch.grad[2], turns it into the gradients [B][E][kGradParams] and [B].
template <typename T>
static int ensure_tbar_scratch(lynx_ctx* ctx, const lynx_lattice* lat) {
  const size_t B = (size_t)lat->batch, S = (size_t)lat->n_steps, E = (size_t)lat->n_elems;
  if (const int rc = ensure_scratch(ctx, ctx->scratch.grad[1], B * S * kGradStride * sizeof(T))) return rc;
  return ensure_scratch(ctx, ctx->scratch.grad[2], B * (2 * E + S + 1) * 49 * sizeof(T));
}

// `merged`: the sweep walked [run, cavity] pairs as one unit each, k_build_bwd takes their cotangents apart again.
// `pool_in_args`: the parameters travel in the kernel's arguments (the caller has not brought d_pool up to date).
template <typename T>
static int launch_build_bwd(lynx_ctx* ctx, lynx_lattice* lat, const void* d_energy_in, void* d_grad_params, void* d_grad_energy_in,
                            int merged, bool pool_in_args) {
  const int64_t B = lat->batch;
  const int32_t S = lat->n_steps, E = lat->n_elems;
  int rc;
  if ((rc = ensure_bwd_tasks(ctx, lat))) return rc;
  // the kind-sorted task list and the elements' kinds, then -- while they fit -- the maps and prefix products
  size_t lds = build_bwd_lds_fixed<T>(S, E);
  const size_t maps_bytes = (size_t)(2 * E + S + 1) * 49 * sizeof(T);
  const int maps_in_lds = lds + maps_bytes <= kBwdMapsLdsBytes;
  if (maps_in_lds) lds += maps_bytes;
  const auto launch = [&](const auto&... pool) -> int {
    const auto kernel = build_bwd_kernel<T>(pool...);
    if (const int refused = allow_lds(ctx, kernel, lds)) return refused;
    HIP_TRY(ctx, hipMemsetAsync(d_grad_params, 0, (size_t)B * E * kGradParams * sizeof(T), ctx->stream));
    hipLaunchKernelGGL(kernel, dim3((unsigned)B), dim3(256), lds, ctx->stream, pool..., dev_view(lat), (const T*)d_energy_in,
                       (T*)ctx->scratch.grad[1].buf, (T*)ctx->scratch.grad[2].buf, (T*)d_grad_params, (T*)d_grad_energy_in, merged,
                       maps_in_lds, lat->d_bwd_tasks, lat->n_bwd_tasks);
    HIP_TRY(ctx, hipGetLastError());
    return LYNX_OK;
  };
  return with_pool_form<T>(lat, pool_in_args, launch);
}

// The sweep over the particles (k_track_bwd, k_track_bwd_units, k_track_bwd_inject): a workgroup walks `tiles_per_wg`
// tiles of kTrackThreads lanes, W particles per lane, `chunks` workgroups per sample; its LDS holds the exchange buffer
// and the waves' per-step sums.
template <typename T, int W>
static size_t bwd_stream_lds_bytes(int32_t S) {
  return ((size_t)4 * ExRows<W>::value * ExGeom<T, W>::kPitch + (size_t)4 * S * bwd_acc_stride<T>(S)) * sizeof(T);
}

// (the 64 units fit: 64 float64 steps at the narrow stride take 161088 bytes, 128 float32 steps 162752)
static int refuse_bwd_stream_lds(lynx_ctx* ctx, const char* what, int32_t S, size_t lds) {
  if (lds <= 160 * 1024) return LYNX_OK;
  return fail(ctx, LYNX_ERR_INVALID,
              std::string(what) + "LDS budget exceeded: " + std::to_string(S) + " steps need " + std::to_string(lds) +
                  " bytes of the 163840 per workgroup (split the lattice)");
}

struct BwdSweepPlan {
  int64_t ntiles, chunks, tiles_per_wg;
  size_t lds;
};

template <typename T, int W>
static BwdSweepPlan plan_bwd_sweep(const lynx_ctx* ctx, int64_t B, int64_t N, int32_t S, BwdArgs* a) {
  BwdSweepPlan p;
  const int64_t cus = compute_units(ctx);
  p.ntiles = (N + kTrackThreads * W - 1) / (kTrackThreads * W);
  p.chunks = std::max<int64_t>(1, std::min<int64_t>(p.ntiles, ((int64_t)kBwdWgsPerCu * cus + B - 1) / B));
  p.tiles_per_wg = (p.ntiles + p.chunks - 1) / p.chunks;
  p.chunks = (p.ntiles + p.tiles_per_wg - 1) / p.tiles_per_wg;
  p.lds = bwd_stream_lds_bytes<T, W>(S);
  a->n_particles = N;
  a->chunks = (int32_t)p.chunks;
  a->tiles_per_wg = (int32_t)p.tiles_per_wg;
  return p;
}

// The units the sweep parks the (s, delta) of: every step one, or (`merge`) a run and the cavity behind it together, at
// the cavity's slot, in the merged form of the forward kernel; `observers`: the observer steps are numbered.  Returns
// whether there is a pair -- the `merged` of the step table and of k_build_bwd --, or -1: more units than the kernels park.
static int plan_bwd_units(const lynx_lattice* lat, bool merge, bool observers, BwdArgs* a) {
  const int32_t S = lat->n_steps;
  int merged = 0;
  a->n_units = a->n_observers = a->out_chunks = a->n_work = a->leave_odd = 0;
  for (int32_t s = 0; s < S; ++s) {
    const bool pair = merge && s + 1 < S && lat->h_steps[s].kind == LYNX_STEP_RUN &&
                      lat->h_steps[s + 1].kind == LYNX_STEP_CAVITY && !(lat->h_steps[s].flags & LYNX_STEP_FLAG_OBSERVE);
    if (pair) merged = 1, ++s;
    if (a->n_units >= kBwdGroup * kBwdMaxGroups || s > 255) return -1;
    const bool observed = observers && (lat->h_steps[s].flags & LYNX_STEP_FLAG_OBSERVE);
    a->unit_observer[a->n_units] = observed ? (unsigned char)(++a->n_observers) : 0;
    a->unit_slot[a->n_units++] = (unsigned char)s;
  }
  for (int u = a->n_units; u < kBwdGroup * kBwdMaxGroups; ++u) a->unit_slot[u] = a->unit_observer[u] = 0;
  return merged;
}

// the workgroups' partial sums [B][chunks][S][kGradStride] -> T_bar in scratch.grad[1]
template <typename T>
static int reduce_tbar(lynx_ctx* ctx, const T* partials, int64_t B, int32_t S, int64_t chunks) {
  if (chunks >= 16) {
    hipLaunchKernelGGL(k_reduce_tbar<T>, dim3((unsigned)(B * S)), dim3(256), 0, ctx->stream, partials, (int)chunks, (int)S,
                       (T*)ctx->scratch.grad[1].buf);
  } else {  // four rows (sample, step) per wave
    const int64_t rows = B * S;
    hipLaunchKernelGGL((k_reduce_tbar_rows<T, 4>), dim3((unsigned)((rows + 15) / 16)), dim3(256), 0, ctx->stream, partials,
                       (int)chunks, (int)S, rows, (T*)ctx->scratch.grad[1].buf);
  }
  HIP_TRY(ctx, hipGetLastError());
  return LYNX_OK;
}

// What a reverse entry point writes for the caller: the gradients of the parameters, of the incoming energy and (if it
// has them: a null block is nothing) of the incoming moments, and what `more` it has.
static std::array<Written, 5> reverse_writes(const lynx_lattice* lat, void* d_grad_params, void* d_grad_energy_in, void* d_grad_mu_in,
                                             void* d_grad_cov_in, Written more = {nullptr, 0}) {
  const size_t es = dtype_size(lat->dtype);
  return {{{d_grad_params, (size_t)lat->batch * lat->n_elems * kGradParams * es},
           {d_grad_energy_in, (size_t)lat->batch * es},
           {d_grad_mu_in, (size_t)lat->batch * 7 * es},
           {d_grad_cov_in, (size_t)lat->batch * 49 * es},
           more}};
}

// -- the stages of track_backward_t --

// The step table and, for the structured kernel, the unit records the sweep reads.
struct BwdTable {
  const void* d_steps = nullptr;
  float* d_units = nullptr;  // null: no sample takes k_track_bwd_units
  float* d_extras = nullptr;
  bool all_proposed_u = false;  // the plan proposes class U for every unit: only a sample with a non-finite map is left to k_track_bwd
  int reused_slot = -1;         // the slot of the forward call's table, if that is the one read
};

// float32 packed pairs: samples whose units all have class U take the structured reverse kernel (lynx_grad_units.hpp),
// if the lattice's units plan is the sweep's (LYNX_BWD_UNITS=0: never).  Its records go to the reverse pass's own scratch.
static int bwd_units_records(lynx_ctx* ctx, lynx_lattice* lat, int merged, const BwdArgs& a, BwdTable* t) {
  int rc;
  if (!ctx->knobs.bwd_units) return LYNX_OK;
  if ((rc = ensure_units_plan(ctx, lat, merged != 0))) return rc;
  const UnitPlan& up = lat->units[merged ? 1 : 0];
  // (the structured kernel parks the (s, delta) entering every unit in registers: up to kBwdUnitsMax units)
  bool same = lat->units_ok[merged ? 1 : 0] && up.n_units == a.n_units && a.n_units <= kBwdUnitsMax;
  for (int u = 0; same && u < a.n_units; ++u) same = up.slot[u] == a.unit_slot[u];
  if (!same) return LYNX_OK;
  const int64_t n = lat->batch * a.n_units;
  if ((rc = ensure_scratch(ctx, ctx->scratch.units_bwd[0], (size_t)n * kUnitStride * sizeof(float))) ||
      (rc = ensure_scratch(ctx, ctx->scratch.units_bwd[1], (size_t)n * kUnitExtraStride * sizeof(float))))
    return rc;
  t->d_units = (float*)ctx->scratch.units_bwd[0].buf;
  t->d_extras = (float*)ctx->scratch.units_bwd[1].buf;
  t->all_proposed_u = true;
  for (int u = 0; u < up.n_units; ++u) t->all_proposed_u = t->all_proposed_u && up.cls[u] == kClassU;
  return LYNX_OK;
}

// The forward call this reverse pass belongs to has built exactly this table (and these unit records) a moment ago: read
// them where they are (LYNX_BWD_REUSE_TABLE=0: never).  Otherwise build them into the reverse pass's own.
template <typename T>
static int bwd_table(lynx_ctx* ctx, lynx_lattice* lat, const void* d_energy_in, int merged, size_t steps_bytes, BwdTable* t) {
  std::unique_lock<std::mutex> table_lock(ctx->mu);
  const lynx_ctx::FwdTable ft = ctx->fwd_table;
  table_lock.unlock();
  const bool reuse = ctx->knobs.bwd_reuse_table && ft.valid && ft.lat == lat && ft.version == lat->version &&
                     ft.energy == d_energy_in && ft.seq == ctx->seq && ft.merged == merged &&
                     ctx->scratch.steps[ft.slot].bytes >= steps_bytes;
  if (!reuse) {
    t->d_steps = ctx->scratch.steps[lynx_ctx::kTableBwd].buf;
    return launch_build<T>(ctx, lat, ctx->stream, d_energy_in, ctx->scratch.steps[lynx_ctx::kTableBwd].buf, nullptr, merged, false,
                           t->d_units, t->d_extras);
  }
  t->reused_slot = ft.slot;
  t->d_steps = ctx->scratch.steps[ft.slot].buf;
  if (t->d_units && ft.units) {
    t->d_units = (float*)ctx->scratch.units[ft.slot].buf;
    t->d_extras = (float*)ctx->scratch.units[lynx_ctx::kTableSlots + ft.slot].buf;
  } else if (t->d_units) {  // the forward call walked the table itself (a single-map program): the records from its rows
    if constexpr (sizeof(T) == 4) return launch_pack_units(ctx, lat, merged, ctx->stream, t->d_steps, t->d_units, t->d_extras);
  }
  return LYNX_OK;
}

// The streaming launches: the structured kernel for the samples whose units all have class U, then the dense one.
template <typename T, typename Z>
static int launch_bwd_sweep(lynx_ctx* ctx, lynx_lattice* lat, const BwdArgs& a, const BwdSweepPlan& p, const BwdTable& t,
                            const void* d_p_in, const double* d_moments_fwd, const double* d_grad_moments, void* d_grad_p_in,
                            const double* d_grad_observations) {
  constexpr int W = LaneOf<Z>::W;
  const int64_t B = lat->batch;
  const int32_t S = lat->n_steps;
  int rc;
  if constexpr (W == 2) {
    if (t.d_units) {
      const size_t lds_u = bwd_units_lds_bytes(S);
      const auto launch = [&](auto kernel) -> int {
        if (const int refused = allow_lds(ctx, kernel, lds_u)) return refused;
        hipLaunchKernelGGL(kernel, dim3((unsigned)(B * p.chunks)), dim3(kTrackThreads), lds_u, ctx->stream, a, S, (const float*)d_p_in,
                           (const float*)t.d_units, (const float*)t.d_extras, d_moments_fwd, d_grad_moments,
                           (float*)ctx->scratch.grad[0].buf, (float*)d_grad_p_in);
        HIP_TRY(ctx, hipGetLastError());
        return LYNX_OK;
      };
      if ((rc = a.n_units <= 8 ? launch(k_track_bwd_units<8>) : launch(k_track_bwd_units<kBwdUnitsMax>))) return rc;
    }
  }
  // Next to k_track_bwd_units this kernel is there for the samples that one left: workgroups of the others return at once --
  // 40 us for BASELINE config 5's 40 960 of them, which take 60 KB of LDS each to be placed.  When the plan proposes class
  // U for EVERY unit, only a sample with a non-finite map can be left: ONE workgroup per sample then (it walks all of
  // the sample's tiles, writes row 0 of the sample's partial sums and clears the rest).
  BwdArgs a_dense = a;
  a_dense.n_work = (int32_t)(B * p.chunks);
  int64_t dense_grid = B * p.chunks;
  if (t.d_units && t.all_proposed_u) {
    if (p.chunks > 1) {
      a_dense.out_chunks = (int32_t)p.chunks;
      a_dense.chunks = 1;
      a_dense.tiles_per_wg = (int32_t)p.ntiles;
    }
    a_dense.n_work = (int32_t)B;
    const int64_t cus = compute_units(ctx);
    dense_grid = std::min<int64_t>(B, 2 * cus);  // (and as many workgroups as are resident at once: they look at B / grid samples each)
  }
  hipLaunchKernelGGL((k_track_bwd<T, Z>), dim3((unsigned)dense_grid), dim3(kTrackThreads), p.lds, ctx->stream, dev_view(lat), a_dense,
                     (const T*)d_p_in, (const T*)t.d_steps, d_moments_fwd, d_grad_moments, (T*)ctx->scratch.grad[0].buf,
                     (T*)d_grad_p_in, (const float*)t.d_units, kUnitStride, kUnitClassShift, (int)kClassU, d_grad_observations);
  HIP_TRY(ctx, hipGetLastError());
  return LYNX_OK;
}

// The reverse pass of one track call.  Z: what a lane carries -- one particle, or (float32) two as a packed pair.
template <typename T, typename Z = T>
static int track_backward_t(lynx_ctx* ctx, lynx_lattice* lat, int64_t N, const void* d_energy_in, const void* d_p_in,
                            const double* d_moments_fwd, const double* d_grad_moments, void* d_grad_params,
                            void* d_grad_energy_in, void* d_grad_p_in, const double* d_grad_observations) {
  constexpr int W = LaneOf<Z>::W;
  const int64_t B = lat->batch;
  const int32_t S = lat->n_steps;
  int rc;
  // (k_build_bwd reads the parameters: from its arguments if the lattice's pool travels there, from memory otherwise)
  const bool pool_in_args = lat->prog_pool && ctx->knobs.inline_pool != 0;
  if (!pool_in_args && (rc = sync_pool(ctx, lat))) return rc;
  // the units of the program, and what is refused about them -- here, before anything is built or launched
  // (packed float32 pairs walk [run, cavity] pairs as one unit; LYNX_BWD_MERGE=0: every step on its own)
  BwdArgs a;
  const int merged = plan_bwd_units(lat, W == 2 && ctx->knobs.bwd_merge, true, &a);
  if (merged < 0)
    return fail(ctx, LYNX_ERR_INVALID,
                "lynx_track_particles_backward: " + std::to_string(S) + " steps; this version parks at most " +
                    std::to_string(kBwdGroup * kBwdMaxGroups) + " (merge skippable elements or split the lattice)");
  a.leave_odd = ctx->knobs.bwd_units == 2 ? 1 : 0;
  const BwdSweepPlan p = plan_bwd_sweep<T, W>(ctx, B, N, S, &a);
  if ((rc = refuse_bwd_stream_lds(ctx, "lynx_track_particles_backward: ", S, p.lds))) return rc;
  // the units plan for the structured kernel, then the table: the forward call's, or one built here
  BwdTable t;
  const size_t steps_bytes = (size_t)B * S * LYNX_STEP_STRIDE * sizeof(T);
  if ((rc = ensure_scratch(ctx, ctx->scratch.steps[lynx_ctx::kTableBwd], steps_bytes))) return rc;
  if constexpr (W == 2)
    if ((rc = bwd_units_records(ctx, lat, merged, a, &t))) return rc;
  if ((rc = bwd_table<T>(ctx, lat, d_energy_in, merged, steps_bytes, &t))) return rc;
  // the sweep over the particles -> partial sums [B][chunks][S][kGradStride] in scratch.grad[0] -> T_bar
  if ((rc = allow_lds(ctx, k_track_bwd<T, Z>, p.lds))) return rc;
  if ((int64_t)B * p.chunks > 0x7fffffffLL || (int64_t)B * S > 0x7fffffffLL) return fail(ctx, LYNX_ERR_INVALID, "grid too large");
  if ((rc = ensure_scratch(ctx, ctx->scratch.grad[0], (size_t)B * p.chunks * S * kGradStride * sizeof(T))))
    return rc;
  if ((rc = ensure_tbar_scratch<T>(ctx, lat))) return rc;
  if ((rc = launch_bwd_sweep<T, Z>(ctx, lat, a, p, t, d_p_in, d_moments_fwd, d_grad_moments, d_grad_p_in, d_grad_observations))) return rc;
  if ((rc = reduce_tbar<T>(ctx, (const T*)ctx->scratch.grad[0].buf, B, S, p.chunks))) return rc;
  if constexpr (W == 2) {
    if (t.d_units) {  // class-U samples: the units' transverse blocks from the sample's S_x, S_y (lynx_grad_units.hpp)
      hipLaunchKernelGGL(k_finish_tbar_units, dim3((unsigned)B), dim3(64), 0, ctx->stream, a, S, (const float*)t.d_units,
                         (float*)ctx->scratch.grad[1].buf);
      HIP_TRY(ctx, hipGetLastError());
    }
  }
  if (t.reused_slot >= 0) {  // the forward call's table slot has been read up to here: its next build waits for this, too
    HIP_TRY(ctx, ctx->order.read_until_here(t.reused_slot, ctx->stream));
  }
  return launch_build_bwd<T>(ctx, lat, d_energy_in, d_grad_params, d_grad_energy_in, merged, pool_in_args);
}

int lynx_track_particles_backward(lynx_ctx* ctx, lynx_lattice* lat, int64_t n_particles, const void* d_energy_in,
                                  const void* d_p_in, const double* d_moments_fwd, const double* d_grad_moments,
                                  void* d_grad_params, void* d_grad_energy_in, void* d_grad_p_in,
                                  const double* d_grad_observations) {
  LYNX_MAIN_ENTRY(ctx);
  if (!lat || !d_energy_in || !d_p_in || !d_moments_fwd || !d_grad_moments || !d_grad_params || !d_grad_energy_in)
    return fail(ctx, LYNX_ERR_INVALID, "null argument");
  if (n_particles <= 0 || lat->n_steps <= 0) return fail(ctx, LYNX_ERR_INVALID, "empty program or beam");
  if (d_grad_observations && lat->n_observers == 0)
    return fail(ctx, LYNX_ERR_INVALID, "d_grad_observations given, but the program has no observer step");
  LYNX_MAIN_WRITES(ctx, kFeedsBuild, {});  // (what it writes: behind the pass, below)
  if (const int rc = join_side(ctx)) return rc;  // d_moments_fwd is what a reduction on the side stream writes
  const auto pass = lat->dtype == LYNX_F64   ? track_backward_t<double, double>
                    : ctx->knobs.bwd_pairs ? track_backward_t<float, lynx_f32x2>
                                           : track_backward_t<float, float>;
  const int rc = pass(ctx, lat, n_particles, d_energy_in, d_p_in, d_moments_fwd, d_grad_moments, d_grad_params, d_grad_energy_in,
                      d_grad_p_in, d_grad_observations);
  // The gradients it wrote for the caller, said AFTER the pass: `wrote` invalidates the FwdTable if a block overlaps the
  // forward call's incoming energy, and the pass reads that table -- said up front, it would build its own instead
  // (the other reverse passes read no FwdTable: they say it up front).
  caller_blocks_written(ctx, kFeedsNoBuild,
                        reverse_writes(lat, d_grad_params, d_grad_energy_in, nullptr, nullptr,
                                       {d_grad_p_in, (size_t)lat->batch * n_particles * 7 * dtype_size(lat->dtype)}));
  return rc;
}

template <typename T>
static int moments_backward_t(lynx_ctx* ctx, lynx_lattice* lat, const void* d_energy_in, const void* d_mu_in,
                              const void* d_cov_in, const void* d_mu_bar, const void* d_cov_bar, void* d_grad_params,
                              void* d_grad_energy_in, void* d_grad_mu_in, void* d_grad_cov_in) {
  const int64_t B = lat->batch;
  const int32_t S = lat->n_steps;
  int rc;
  if ((rc = sync_pool(ctx, lat))) return rc;  // (k_moments_bwd and k_build_bwd read the parameters from memory)
  if ((rc = ensure_scratch(ctx, ctx->scratch.steps[lynx_ctx::kTableBwd], (size_t)B * S * LYNX_STEP_STRIDE * sizeof(T))))
    return rc;
  if ((rc = launch_build<T>(ctx, lat, ctx->stream, d_energy_in, ctx->scratch.steps[lynx_ctx::kTableBwd].buf, nullptr))) return rc;
  if ((rc = ensure_scratch(ctx, ctx->scratch.grad[0], (size_t)B * (S + 1) * 56 * sizeof(T))))
    return rc;
  if ((rc = ensure_tbar_scratch<T>(ctx, lat))) return rc;
  hipLaunchKernelGGL(k_moments_bwd<T>, dim3((unsigned)B), dim3(64), 0, ctx->stream, dev_view(lat), (const T*)ctx->scratch.steps[lynx_ctx::kTableBwd].buf,
                     (const T*)d_mu_in, (const T*)d_cov_in, (const T*)d_mu_bar, (const T*)d_cov_bar,
                     (T*)ctx->scratch.grad[0].buf, (T*)ctx->scratch.grad[1].buf, (T*)d_grad_mu_in, (T*)d_grad_cov_in);
  HIP_TRY(ctx, hipGetLastError());
  return launch_build_bwd<T>(ctx, lat, d_energy_in, d_grad_params, d_grad_energy_in, 0, false);
}

int lynx_track_moments_backward(lynx_ctx* ctx, lynx_lattice* lat, const void* d_energy_in, const void* d_mu_in,
                                const void* d_cov_in, const void* d_mu_bar, const void* d_cov_bar,
                                void* d_grad_params, void* d_grad_energy_in, void* d_grad_mu_in,
                                void* d_grad_cov_in) {
  LYNX_MAIN_ENTRY(ctx);
  if (!lat || !d_energy_in || !d_mu_in || !d_cov_in || !d_mu_bar || !d_cov_bar || !d_grad_params ||
      !d_grad_energy_in || !d_grad_mu_in || !d_grad_cov_in)
    return fail(ctx, LYNX_ERR_INVALID, "null argument");
  if (lat->n_steps <= 0) return fail(ctx, LYNX_ERR_INVALID, "empty program");
  if (lat->batch > 0x7fffffffLL) return fail(ctx, LYNX_ERR_INVALID, "batch too large");
  LYNX_MAIN_WRITES(ctx, kFeedsBuild, reverse_writes(lat, d_grad_params, d_grad_energy_in, d_grad_mu_in, d_grad_cov_in));
  return with_dtype(lat->dtype, [&](auto zero) {
    return moments_backward_t<decltype(zero)>(ctx, lat, d_energy_in, d_mu_in, d_cov_in, d_mu_bar, d_cov_bar, d_grad_params,
                                              d_grad_energy_in, d_grad_mu_in, d_grad_cov_in);
  });
}

int lynx_moments(lynx_ctx* ctx, int dtype, int64_t batch, int64_t n_particles, const void* d_p,
                 double* d_moments_out, int32_t covariance) {
  LYNX_MAIN_ENTRY(ctx);
  if (!d_p || !d_moments_out) return fail(ctx, LYNX_ERR_INVALID, "null argument");
  if (batch <= 0 || n_particles <= 0) return fail(ctx, LYNX_ERR_INVALID, "bad shape");
  LYNX_MAIN_WRITES(ctx, kFeedsNoBuild, {});  // (track_particles_t says what it writes)
  LatticeDev lv;
  memset(&lv, 0, sizeof(lv));
  lv.batch = batch;
  return with_dtype(dtype, [&](auto zero) {
    return track_particles_t<decltype(zero)>(ctx, nullptr, lv, batch, n_particles, nullptr, d_p, nullptr, nullptr, d_moments_out,
                                             covariance ? LYNX_TRACK_COVARIANCE : LYNX_TRACK_MOMENTS);
  });
}

// ---- ParameterBeam ---------------------------------------------------------------------

template <typename T>
static int launch_track_moments(lynx_ctx* ctx, lynx_lattice* lat, const void* d_energy_in, const void* d_mu_in,
                                const void* d_cov_in, void* d_mu_out, void* d_cov_out, void* d_energy_out) {
  if constexpr (sizeof(T) == 4)  // (float64: 98 VGPRs of covariance per lane -- the compiler spills; workgroup form below)
  if (lat->n_steps > 0 && lat->batch >= ctx->knobs.lanes_build_min_batch) {
    // large batches: lanes = samples all the way (step table from the lanes build, then one lane per sample)
    int rc;
    const size_t need = (size_t)lat->batch * lat->n_steps * LYNX_STEP_STRIDE * sizeof(T);
    if ((rc = ensure_scratch(ctx, ctx->scratch.steps[lynx_ctx::kTablePb], need))) return rc;
    if ((rc = launch_build<T>(ctx, lat, ctx->stream, d_energy_in, ctx->scratch.steps[lynx_ctx::kTablePb].buf, nullptr, 0))) return rc;
    hipLaunchKernelGGL(k_apply_moments_lanes<T>, dim3((unsigned)((lat->batch + 63) / 64)), dim3(64), apply_moments_lds<T>(),
                       ctx->stream, dev_view(lat), (const T*)ctx->scratch.steps[lynx_ctx::kTablePb].buf, (const T*)d_mu_in, (const T*)d_cov_in,
                       (T*)d_mu_out, (T*)d_cov_out, (T*)d_energy_out);
    HIP_TRY(ctx, hipGetLastError());
    return LYNX_OK;
  }
  // one workgroup per sample: one wave for big batches, four otherwise -- with chunks of up to 128 elements when the
  // batch leaves most of the GPU idle and the depth of the tree is what the call waits for (build_shape)
  const unsigned threads = lat->batch <= 4096 ? 256u : 64u;
  const int chunk = fit_build_chunk<T>(build_shape<T>(ctx, lat, /* underneath */ false, /* short_float32 */ false), lat, kMomentsTailScalars);
  const size_t lds = build_lds_layout(chunk, (size_t)lat->n_steps, sizeof(T), kMomentsTailScalars).total;
  // (the cavity flags -- none where the pool travels in the arguments: such a lattice has no cavity -- come behind
  // sync_pool and allow_lds here, in launch_build in front of both: each launcher keeps its own order)
  const auto launch = [&](const auto&... pool) -> int {
    const auto kernel = track_moments_kernel<T>(pool...);
    if constexpr (sizeof...(pool) == 0)
      if (const int stale = sync_pool(ctx, lat)) return stale;
    if (const int refused = allow_lds(ctx, kernel, lds)) return refused;
    if constexpr (sizeof...(pool) == 0)
      if (const int failed = launch_cavity_flags<T>(ctx, lat, ctx->stream, d_energy_in)) return failed;
    hipLaunchKernelGGL(kernel, dim3((unsigned)lat->batch), dim3(threads), lds, ctx->stream, pool..., dev_view(lat), (const T*)d_energy_in,
                       (const T*)d_mu_in, (const T*)d_cov_in, (T*)d_mu_out, (T*)d_cov_out, (T*)d_energy_out, chunk);
    HIP_TRY(ctx, hipGetLastError());
    return LYNX_OK;
  };
  return with_pool_form<T>(lat, lat->prog_pool && ctx->knobs.inline_pool, launch);
}

int lynx_track_moments(lynx_ctx* ctx, lynx_lattice* lat, const void* d_energy_in, const void* d_mu_in,
                       const void* d_cov_in, void* d_mu_out, void* d_cov_out, void* d_energy_out) {
  LYNX_MAIN_ENTRY(ctx);
  if (!lat || !d_energy_in || !d_mu_in || !d_cov_in || !d_mu_out || !d_cov_out)
    return fail(ctx, LYNX_ERR_INVALID, "null argument");
  if (lat->batch > 0x7fffffffLL) return fail(ctx, LYNX_ERR_INVALID, "batch too large");
  const size_t es = dtype_size(lat->dtype);
  LYNX_MAIN_WRITES(ctx, kFeedsBuild, {{d_energy_out, (size_t)lat->batch * es},
                                      {d_mu_out, (size_t)lat->batch * 7 * es},
                                      {d_cov_out, (size_t)lat->batch * 49 * es}});
  return with_dtype(lat->dtype, [&](auto zero) {
    return launch_track_moments<decltype(zero)>(ctx, lat, d_energy_in, d_mu_in, d_cov_in, d_mu_out, d_cov_out, d_energy_out);
  });
}

// ---- beam trace: the moments at every element of the lattice ---------------------------------

// The table of a program whose every element is a step of its own, [B][E][64], in the trace's own slot (the ring of
// the forward calls -- and with it the table a reverse pass may still want -- is left alone), on the main stream.
template <typename T>
static int trace_table(lynx_ctx* ctx, lynx_lattice* lat, const void* d_energy_in) {
  int rc;
  const size_t need = std::max<size_t>(1, (size_t)lat->batch * lat->n_steps) * LYNX_STEP_STRIDE * sizeof(T);
  if ((rc = ensure_scratch(ctx, ctx->scratch.steps[lynx_ctx::kTableTrace], need)))
    return rc;
  if (lat->n_steps == 0) return LYNX_OK;
  // no limit on the number of elements: where the workgroup build's table would not fit its LDS, lanes = samples
  // (by the chunk of build_shape as it stands, not the one launch_build would halve it to)
  const size_t lds = build_lds_layout(build_shape<T>(ctx, lat, false, true), (size_t)lat->n_steps, sizeof(T), 0).total;
  return launch_build<T>(ctx, lat, ctx->stream, d_energy_in, ctx->scratch.steps[lynx_ctx::kTableTrace].buf, nullptr, 0, false, nullptr,
                         nullptr, lds > (size_t)64 * 1024);
}

// The apertures of a trace with losses as the host hands them over.
struct TraceApertures {
  int32_t count;
  const int32_t* pairs;  // [count][2]: step, elliptical
  const void* d_limits;
  int64_t limit_stride;
  int32_t* d_lost_at;
};

// The screens of a trace as the host hands them over.
struct TraceScreenList {
  int32_t count;
  const int32_t* rows;  // [count][3]: step, nx, ny
  const void* d_edges;
  const void* d_misalignment;
  int64_t misalignment_stride;
  int32_t* d_images;
  int64_t cells;  // sum of ny nx (track_particles_along fills it in)
};

// The chosen particles of a trace with trajectories as the host hands them over.
struct TraceChosen {
  int64_t count;
  const int64_t* d_indices;  // [count]
  void* d_trajectories;      // [B][P][count][7]
  int32_t* d_lost_in;        // [B][count] or null
};

// TraceLosses.plan of this call on the device (either list may be null).  The plan is uploaded when it differs from the
// one that is there (a scan calls with the same lattice over and over); the wait that upload needs is paid once per
// lattice structure.
static int trace_plan(lynx_ctx* ctx, int32_t S, const TraceApertures* ap, const TraceScreenList* sc) {
  std::vector<int64_t> plan(std::max<size_t>(1, (size_t)S + 4 * (size_t)(sc ? sc->count : 0)), -1);
  for (int32_t k = 0; ap && k < ap->count; ++k) plan[ap->pairs[2 * k]] = ((int64_t)k << 2) | (ap->pairs[2 * k + 1] ? 2 : 0);
  int64_t edge = 0, cell = 0;
  for (int32_t k = 0; sc && k < sc->count; ++k) {
    const int64_t nx = sc->rows[3 * k + 1], ny = sc->rows[3 * k + 2];
    plan[sc->rows[3 * k]] = ((int64_t)k << 2) | 1;
    int64_t* row = plan.data() + S + 4 * (size_t)k;
    row[0] = nx, row[1] = ny, row[2] = edge, row[3] = cell;
    edge += nx + ny + 2;
    cell += nx * ny;
  }
  const size_t need = plan.size() * sizeof(int64_t);
  const bool fresh = ctx->scratch.trace_plan.bytes < need;
  int rc;
  if ((rc = ensure_scratch(ctx, ctx->scratch.trace_plan, need))) return rc;
  if (fresh || plan != ctx->trace_plan) {
    ctx->trace_plan.clear();
    HIP_TRY(ctx, hipMemcpyAsync(ctx->scratch.trace_plan.buf, plan.data(), need, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, sync_main(ctx));  // (kernels of earlier calls have read the old plan; the host vector is ours again)
    ctx->trace_plan.swap(plan);
  }
  return LYNX_OK;
}

// `count`: N, or negative for the point's own count (k_trace_finalize).
template <typename T>
static int launch_trace_finalize(lynx_ctx* ctx, int64_t B, int32_t P, int64_t waves, int64_t count, double* d_trace_out) {
  // (few waves per sample: 8 groups of them; hundreds to thousands -- few samples of many particles: 32)
  if (waves > 256)
    hipLaunchKernelGGL((k_trace_finalize<T, 1024>), dim3((unsigned)(B * P)), dim3(1024), 0, ctx->stream,
                       (const double*)ctx->scratch.trace[0].buf, (const T*)ctx->scratch.trace[1].buf, (int)waves, (int)P, count, d_trace_out);
  else
    hipLaunchKernelGGL((k_trace_finalize<T, 256>), dim3((unsigned)(B * P)), dim3(256), 0, ctx->stream,
                       (const double*)ctx->scratch.trace[0].buf, (const T*)ctx->scratch.trace[1].buf, (int)waves, (int)P, count, d_trace_out);
  HIP_TRY(ctx, hipGetLastError());
  return LYNX_OK;
}

// Waves per sample of a streaming pass over N particles that leaves `points` records per sample and wave: enough of them
// to fill the GPU three waves per SIMD deep over the whole batch, whole workgroups of four, never more than there are
// tiles -- and few enough for the slabs (256 bytes per wave and point) to stay below 1 GiB.  The plan depends on the
// shapes alone: the same call adds the same numbers in the same order.  (The survivor sets of lynx_moments_by_loss, at
// most 16 "points", never meet the cap, which they were planned without: more than one wave per sample means B < 12 CUs,
// the cap is then at least 2^22 / (16 B) = 262144 / B waves, and the first bound asks for fewer than 24 CUs / B -- less
// on any GPU of fewer than 10 000 CUs.)
struct TraceWavePlan {
  int64_t waves, tiles_per_wave;
};
static TraceWavePlan trace_wave_plan(const lynx_ctx* ctx, int64_t B, int64_t N, int U /* particles per lane */, int64_t points) {
  const int64_t cus = compute_units(ctx);
  const int64_t tiles = (N + 64 * U - 1) / (64 * U);
  int64_t waves = std::max<int64_t>(1, (cus * 12 + B - 1) / B);
  const int64_t slab_cap = std::max<int64_t>(1, ((int64_t)1 << 30) / (B * points * kTraceSlab * (int64_t)sizeof(double)));
  waves = std::min(std::min(waves, tiles), slab_cap);
  const int64_t tiles_per_wave = (tiles + waves - 1) / waves;
  return {((tiles + tiles_per_wave - 1) / tiles_per_wave + 3) / 4 * 4, tiles_per_wave};
}

// `ap`: the apertures of a trace with losses (null: none, and the records stand for N particles each); `sc`: the
// screens (null: none); `tj`: the chosen particles of a trace with trajectories (null: none -- the launches are then
// the very ones they were before there was such a list).
template <typename T>
static int track_particles_along_t(lynx_ctx* ctx, lynx_lattice* lat, int64_t N, const void* d_energy_in, const void* d_p_in,
                                   void* d_p_out, void* d_energy_trace, double* d_trace_out, int flags,
                                   const TraceApertures* ap, const TraceScreenList* sc, const TraceChosen* tj) {
  constexpr int U = sizeof(T) == 4 ? 4 : 2;  // particles per lane (float32: two packed pairs)
  const int64_t B = lat->batch;
  const int32_t S = lat->n_steps, P = S + 1;
  int rc;
  if ((rc = trace_table<T>(ctx, lat, d_energy_in))) return rc;
  const auto [waves, tiles_per_wave] = trace_wave_plan(ctx, B, N, U, P);
  if (B * (waves / 4) > 0x7fffffffLL || B * P > 0x7fffffffLL || tiles_per_wave > 0x7fffffffLL)
    return fail(ctx, LYNX_ERR_INVALID, "beam trace: batch x points too large for one launch");
  if ((rc = ensure_scratch(ctx, ctx->scratch.trace[0], (size_t)B * waves * P * kTraceSlab * sizeof(double))) ||
      (rc = ensure_scratch(ctx, ctx->scratch.trace[1], (size_t)B * P * kTraceRef * sizeof(T))))
    return rc;
  TraceArgs a{};
  a.n_particles = N;
  a.in_stride = (flags & LYNX_TRACK_SHARED_INPUT) ? 0 : N * 7;
  a.waves = (int32_t)waves;
  a.tiles_per_wave = (int32_t)tiles_per_wave;
  a.store = d_p_out ? 1 : 0;
  a.points = P;
  const T* table = (const T*)ctx->scratch.steps[lynx_ctx::kTableTrace].buf;
  const T* ref = (const T*)ctx->scratch.trace[1].buf;
  double* slabs = (double*)ctx->scratch.trace[0].buf;
  if ((ap || sc) && (rc = trace_plan(ctx, S, ap, sc))) return rc;
  // a trace with screens and without an aperture loses nobody: its records are the plain trace's (slot 35 = N)
  const bool counted = ap && (!sc || ap->count > 0);
  const TraceLosses loss{(const int64_t*)ctx->scratch.trace_plan.buf, counted ? ap->d_limits : nullptr, counted ? ap->limit_stride : 0,
                         ap ? ap->d_lost_at : nullptr};
  hipLaunchKernelGGL(k_trace_reference<T>, dim3((unsigned)B), dim3(64), 0, ctx->stream, dev_view(lat), table, (const T*)d_energy_in,
                     (const T*)d_p_in, a.in_stride, N, counted ? loss.plan : nullptr, (const T*)loss.limits, loss.limit_stride,
                     (T*)ctx->scratch.trace[1].buf, (T*)d_energy_trace);
  HIP_TRY(ctx, hipGetLastError());
  // (on the context's stream: a null-stream memset does not wait for what this stream still runs)
  if (sc) HIP_TRY(ctx, hipMemsetAsync(sc->d_images, 0, (size_t)B * sc->cells * sizeof(int32_t), ctx->stream));
  if (ap && ap->d_lost_at)  // every byte 0xff: -1, "survivor"; the kernel writes the cells of the lost
    HIP_TRY(ctx, hipMemsetAsync(ap->d_lost_at, 0xff, (size_t)B * N * sizeof(int32_t), ctx->stream));
  if (tj && tj->d_lost_in)
    HIP_TRY(ctx, hipMemsetAsync(tj->d_lost_in, 0xff, (size_t)B * tj->count * sizeof(int32_t), ctx->stream));
  const dim3 grid((unsigned)(B * (waves / 4)));
  if (sc) {
    const TraceScreens scr{sc->d_edges, sc->d_misalignment, sc->misalignment_stride, sc->d_images, sc->cells};
    hipLaunchKernelGGL((k_trace_particles_screens<T, U>), grid, dim3(256), 0, ctx->stream, a, S, table, ref, (const T*)d_p_in,
                       (T*)d_p_out, slabs, loss, scr);
  } else if (ap) {
    hipLaunchKernelGGL((k_trace_particles_losses<T, U>), grid, dim3(256), 0, ctx->stream, a, S, table, ref, (const T*)d_p_in,
                       (T*)d_p_out, slabs, loss);
  } else {
    hipLaunchKernelGGL((k_trace_particles<T, U>), grid, dim3(256), 0, ctx->stream, a, S, table, ref, (const T*)d_p_in,
                       (T*)d_p_out, slabs);
  }
  HIP_TRY(ctx, hipGetLastError());
  if (tj) {  // behind the particle kernel, on its stream: the same table, the same plan, p_in alone
    constexpr int64_t kChosenTile = sizeof(T) == 4 ? 128 : 64;
    const TraceTrajectories chosen{tj->d_indices, tj->count, tj->d_trajectories, tj->d_lost_in};
    hipLaunchKernelGGL(k_trace_trajectories<T>, dim3((unsigned)(B * ((tj->count + kChosenTile - 1) / kChosenTile))), dim3(64), 0,
                       ctx->stream, chosen, S, table, (const T*)d_p_in, a.in_stride,
                       (ap || sc) ? (const int64_t*)ctx->scratch.trace_plan.buf : nullptr, (const T*)(ap ? ap->d_limits : nullptr),
                       ap ? ap->limit_stride : (int64_t)0);
    HIP_TRY(ctx, hipGetLastError());
  }
  return launch_trace_finalize<T>(ctx, B, P, waves, counted ? -1 : N, d_trace_out);
}

// The four entry points of the particle trace: the checks, the bookkeeping and the dtype dispatch.  `ap` / `sc` / `tj`
// are the lists of a trace with losses / with screens / with trajectories, null where the entry point has none.
static int track_particles_along(lynx_ctx* ctx, lynx_lattice* lat, int64_t n_particles, const void* d_energy_in,
                                 const void* d_p_in, void* d_p_out, void* d_energy_trace, double* d_trace_out, int flags,
                                 const TraceApertures* ap, TraceScreenList* sc, const TraceChosen* tj = nullptr) {
  LYNX_MAIN_ENTRY(ctx);
  const char* mode = tj ? "beam trace with trajectories: " : sc ? "beam trace with screens: " : ap ? "beam trace with losses: " : "beam trace: ";
  const auto refuse = [&](const char* what) { return fail(ctx, LYNX_ERR_INVALID, std::string(mode) + what); };
  if (!lat || !d_energy_in || !d_p_in || !d_energy_trace || !d_trace_out) return refuse("null argument");
  if (n_particles <= 0) return refuse("n_particles must be > 0");
  if (flags & ~LYNX_TRACK_SHARED_INPUT) return refuse("LYNX_TRACK_SHARED_INPUT is the only flag");
  if ((flags & LYNX_TRACK_SHARED_INPUT) && d_p_in == d_p_out) return refuse("a shared incoming beam cannot be tracked in place");
  if (lat->batch <= 0 || lat->batch > 0x7fffffffLL) return refuse("bad batch");
  if (ap) {
    // (0x1fffffff: a step's code keeps two bits for its flags)
    if (ap->count < 0 || ap->count > 0x1fffffff || (ap->count > 0 && (!ap->pairs || !ap->d_limits))) return refuse("bad aperture list");
    if (ap->limit_stride != 0 && ap->limit_stride != 2 * (int64_t)ap->count)
      return refuse("the limits' sample stride is 0 or 2 * n_apertures");
  }
  if (sc) {
    if (sc->count <= 0 || sc->count > 0x1fffffff || !sc->rows || !sc->d_edges || !sc->d_misalignment || !sc->d_images)
      return refuse("bad screen list");
    if (sc->misalignment_stride != 0 && sc->misalignment_stride != 2 * (int64_t)sc->count)
      return refuse("the misalignments' sample stride is 0 or 2 * n_screens");
  }
  if (tj) {
    if (!tj->d_indices || !tj->d_trajectories) return refuse("null argument");
    if (tj->count < 1) return refuse("n_chosen must be >= 1");
    if (d_p_in == d_p_out) return refuse("the trajectories are read from d_p_in: it cannot be tracked in place");
    // one launch: a workgroup per (sample, 64 chosen particles at the least), the output indexed in int64 bytes
    const int64_t points = (int64_t)lat->n_steps + 1, most = INT64_MAX / (7 * 8);
    if (tj->count > most / lat->batch || tj->count * lat->batch > most / points || lat->batch * ((tj->count + 63) / 64) > 0x7fffffffLL)
      return refuse("batch x points x n_chosen x 7 too large for one launch");
  }
  for (int32_t k = 0; ap && k < ap->count; ++k) {  // lattice order, every step at most once
    const int32_t step = ap->pairs[2 * k];
    if (step < 0 || step >= lat->n_steps || (k > 0 && step <= ap->pairs[2 * k - 2]))
      return refuse("aperture steps must be increasing and inside the program");
  }
  for (int32_t k = 0, a = 0; sc && k < sc->count; ++k) {
    const int32_t step = sc->rows[3 * k], nx = sc->rows[3 * k + 1], ny = sc->rows[3 * k + 2];
    if (step < 0 || step >= lat->n_steps || (k > 0 && step <= sc->rows[3 * k - 3]))
      return refuse("screen steps must be increasing and inside the program");
    while (ap && a < ap->count && ap->pairs[2 * a] < step) ++a;
    if (ap && a < ap->count && ap->pairs[2 * a] == step) return refuse("a step is an aperture or a screen, not both");
    if (nx < 1 || ny < 1) return refuse("a screen has at least one pixel each way");
    sc->cells += (int64_t)nx * ny;
  }
  const size_t es = dtype_size(lat->dtype);
  const size_t B = (size_t)lat->batch, points = (size_t)lat->n_steps + 1;
  LYNX_MAIN_WRITES(ctx, kFeedsBuild, {{d_p_out, B * n_particles * 7 * es},
                                      {d_energy_trace, B * points * es},
                                      {d_trace_out, B * points * LYNX_MOMENT_STRIDE * sizeof(double)},
                                      {ap ? ap->d_lost_at : nullptr, B * n_particles * sizeof(int32_t)},
                                      {sc ? sc->d_images : nullptr, sc ? B * sc->cells * sizeof(int32_t) : 0},
                                      {tj ? tj->d_trajectories : nullptr, tj ? B * points * tj->count * 7 * es : 0},
                                      {tj ? tj->d_lost_in : nullptr, tj ? B * tj->count * sizeof(int32_t) : 0}});
  return with_dtype(lat->dtype, [&](auto zero) {
    return track_particles_along_t<decltype(zero)>(ctx, lat, n_particles, d_energy_in, d_p_in, d_p_out, d_energy_trace, d_trace_out,
                                                   flags, ap, sc, tj);
  });
}

int lynx_track_particles_along(lynx_ctx* ctx, lynx_lattice* lat, int64_t n_particles, const void* d_energy_in,
                               const void* d_p_in, void* d_p_out, void* d_energy_trace, double* d_trace_out, int flags) {
  return track_particles_along(ctx, lat, n_particles, d_energy_in, d_p_in, d_p_out, d_energy_trace, d_trace_out, flags, nullptr, nullptr);
}

int lynx_track_particles_along_losses(lynx_ctx* ctx, lynx_lattice* lat, int64_t n_particles, const void* d_energy_in,
                                      const void* d_p_in, void* d_p_out, void* d_energy_trace, double* d_trace_out, int flags,
                                      int32_t n_apertures, const int32_t* apertures, const void* d_limits,
                                      int64_t limit_stride, int32_t* d_lost_at) {
  const TraceApertures ap{n_apertures, apertures, d_limits, limit_stride, d_lost_at};
  return track_particles_along(ctx, lat, n_particles, d_energy_in, d_p_in, d_p_out, d_energy_trace, d_trace_out, flags, &ap, nullptr);
}

int lynx_track_particles_along_screens(lynx_ctx* ctx, lynx_lattice* lat, int64_t n_particles, const void* d_energy_in,
                                       const void* d_p_in, void* d_p_out, void* d_energy_trace, double* d_trace_out, int flags,
                                       int32_t n_apertures, const int32_t* apertures, const void* d_limits,
                                       int64_t limit_stride, int32_t* d_lost_at, int32_t n_screens, const int32_t* screens,
                                       const void* d_edges, const void* d_misalignment, int64_t misalignment_stride,
                                       int32_t* d_images) {
  const TraceApertures ap{n_apertures, apertures, d_limits, limit_stride, d_lost_at};
  TraceScreenList sc{n_screens, screens, d_edges, d_misalignment, misalignment_stride, d_images, 0};
  return track_particles_along(ctx, lat, n_particles, d_energy_in, d_p_in, d_p_out, d_energy_trace, d_trace_out, flags, &ap, &sc);
}

int lynx_track_particles_along_trajectories(lynx_ctx* ctx, lynx_lattice* lat, int64_t n_particles, const void* d_energy_in,
                                            const void* d_p_in, void* d_p_out, void* d_energy_trace, double* d_trace_out, int flags,
                                            int32_t n_apertures, const int32_t* apertures, const void* d_limits,
                                            int64_t limit_stride, int32_t* d_lost_at, int32_t n_screens, const int32_t* screens,
                                            const void* d_edges, const void* d_misalignment, int64_t misalignment_stride,
                                            int32_t* d_images, int64_t n_chosen, const int64_t* d_indices, void* d_trajectories,
                                            int32_t* d_trajectory_lost_in) {
  // (a negative count: no such list -- the particle kernel is the one the call without trajectories runs)
  const TraceApertures ap{n_apertures, apertures, d_limits, limit_stride, d_lost_at};
  TraceScreenList sc{n_screens, screens, d_edges, d_misalignment, misalignment_stride, d_images, 0};
  const TraceChosen tj{n_chosen, d_indices, d_trajectories, d_trajectory_lost_in};
  return track_particles_along(ctx, lat, n_particles, d_energy_in, d_p_in, d_p_out, d_energy_trace, d_trace_out, flags,
                               n_apertures < 0 ? nullptr : &ap, n_screens < 0 ? nullptr : &sc, &tj);
}

// The moment records of the incoming beam over the nested survivor sets of a trace with losses: the particle trace's
// wave plan with the sets for points, in the trace's own scratch (slabs, reference points), on the main stream.
constexpr int32_t kTraceMaxLossApertures = kMaxLossSets - 1;

template <typename T>
static int moments_by_loss_t(lynx_ctx* ctx, int64_t B, int64_t N, const void* d_p, int flags, int32_t A,
                             const int32_t* d_lost_at, double* d_records_out) {
  constexpr int U = sizeof(T) == 4 ? 4 : 2;
  const int32_t J = A + 1;
  const auto [waves, tiles_per_wave] = trace_wave_plan(ctx, B, N, U, J);
  if (B * (waves / 4) > 0x7fffffffLL || B * J > 0x7fffffffLL || tiles_per_wave > 0x7fffffffLL)
    return fail(ctx, LYNX_ERR_INVALID, "moments by loss: batch too large for one launch");
  int rc;
  if ((rc = ensure_scratch(ctx, ctx->scratch.trace[0], (size_t)B * waves * J * kTraceSlab * sizeof(double))) ||
      (rc = ensure_scratch(ctx, ctx->scratch.trace[1], (size_t)B * J * kTraceRef * sizeof(T))))
    return rc;
  LossSetArgs a{};
  a.n_particles = N;
  a.in_stride = (flags & LYNX_TRACK_SHARED_INPUT) ? 0 : N * 7;
  a.waves = (int32_t)waves;
  a.tiles_per_wave = (int32_t)tiles_per_wave;
  a.sets = J;
  hipLaunchKernelGGL((k_moments_by_loss<T, U>), dim3((unsigned)(B * (waves / 4))), dim3(256), 0, ctx->stream, a, (const T*)d_p,
                     d_lost_at, (double*)ctx->scratch.trace[0].buf, (T*)ctx->scratch.trace[1].buf);
  HIP_TRY(ctx, hipGetLastError());
  return launch_trace_finalize<T>(ctx, B, J, waves, -1, d_records_out);
}

int lynx_moments_by_loss(lynx_ctx* ctx, int dtype, int64_t batch, int64_t n_particles, const void* d_p, int flags,
                         int32_t n_apertures, const int32_t* d_lost_at, double* d_records_out) {
  LYNX_MAIN_ENTRY(ctx);
  const auto refuse = [&](const std::string& what) { return fail(ctx, LYNX_ERR_INVALID, "moments by loss: " + what); };
  if (!d_p || !d_lost_at || !d_records_out) return refuse("null argument");
  if (dtype != LYNX_F32 && dtype != LYNX_F64) return refuse("dtype is LYNX_F32 or LYNX_F64");
  if (n_particles < 1) return refuse("n_particles must be >= 1");
  if (batch <= 0 || batch > 0x7fffffffLL) return refuse("bad batch");
  if (flags & ~LYNX_TRACK_SHARED_INPUT) return refuse("LYNX_TRACK_SHARED_INPUT is the only flag");
  if (n_apertures < 1 || n_apertures > kTraceMaxLossApertures)
    return refuse("n_apertures = " + std::to_string(n_apertures) + ", not 1 .. " + std::to_string(kTraceMaxLossApertures));
  LYNX_MAIN_WRITES(ctx, kFeedsBuild, {{d_records_out, (size_t)batch * (n_apertures + 1) * LYNX_MOMENT_STRIDE * sizeof(double)}});
  return with_dtype(dtype, [&](auto zero) {
    return moments_by_loss_t<decltype(zero)>(ctx, batch, n_particles, d_p, flags, n_apertures, d_lost_at, d_records_out);
  });
}

template <typename T>
static int track_moments_along_t(lynx_ctx* ctx, lynx_lattice* lat, const void* d_energy_in, const void* d_mu_in,
                                 const void* d_cov_in, void* d_mu_trace, void* d_cov_trace, void* d_energy_trace) {
  int rc;
  if ((rc = trace_table<T>(ctx, lat, d_energy_in))) return rc;
  const int64_t B = lat->batch;
  const T* table = (const T*)ctx->scratch.steps[lynx_ctx::kTableTrace].buf;
  hipLaunchKernelGGL(k_trace_energies<T>, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, ctx->stream, dev_view(lat), table,
                     (const T*)d_energy_in, (T*)d_energy_trace);
  HIP_TRY(ctx, hipGetLastError());
  // large float32 batches: lanes = samples (float64: 98 registers of covariance per lane, see launch_track_moments)
  if (sizeof(T) == 4 && B >= ctx->knobs.lanes_build_min_batch) {
    hipLaunchKernelGGL(k_trace_moments_lanes<T>, dim3((unsigned)((B + 63) / 64)), dim3(64), apply_moments_lds<T>(), ctx->stream,
                       dev_view(lat), table, (const T*)d_mu_in, (const T*)d_cov_in, (T*)d_mu_trace, (T*)d_cov_trace);
  } else {
    hipLaunchKernelGGL(k_trace_moments<T>, dim3((unsigned)B), dim3(64), 0, ctx->stream, dev_view(lat), table, (const T*)d_mu_in,
                       (const T*)d_cov_in, (T*)d_mu_trace, (T*)d_cov_trace);
  }
  HIP_TRY(ctx, hipGetLastError());
  return LYNX_OK;
}

int lynx_track_moments_along(lynx_ctx* ctx, lynx_lattice* lat, const void* d_energy_in, const void* d_mu_in,
                             const void* d_cov_in, void* d_mu_trace, void* d_cov_trace, void* d_energy_trace) {
  LYNX_MAIN_ENTRY(ctx);
  if (!lat || !d_energy_in || !d_mu_in || !d_cov_in || !d_mu_trace || !d_cov_trace || !d_energy_trace)
    return fail(ctx, LYNX_ERR_INVALID, "null argument");
  if (lat->batch <= 0 || lat->batch > 0x7fffffffLL) return fail(ctx, LYNX_ERR_INVALID, "bad batch");
  const size_t es = dtype_size(lat->dtype);
  const size_t points = (size_t)lat->batch * ((size_t)lat->n_steps + 1);
  LYNX_MAIN_WRITES(ctx, kFeedsBuild, {{d_energy_trace, points * es}, {d_mu_trace, points * 7 * es}, {d_cov_trace, points * 49 * es}});
  return with_dtype(lat->dtype, [&](auto zero) {
    return track_moments_along_t<decltype(zero)>(ctx, lat, d_energy_in, d_mu_in, d_cov_in, d_mu_trace, d_cov_trace, d_energy_trace);
  });
}

// ---- reverse pass of the beam trace: gradients of the moments at every point -----------------

// The trace's reverse passes refuse longer programs.  k_build_bwd once dealt a program's steps one to each of its 256
// threads; it walks them in strided loops now, but no sweep of the trace has run beyond 256 points and the header states
// the refusal: the limit stays.
constexpr int32_t kTraceBwdMaxSteps = 256;

// What the entry points share.  trace_backward_begin: the trace table and the scratch of T_bar and of k_build_bwd;
// trace_backward_finish: k_build_bwd on the "every element a step of its own" program over the T_bar a sweep left in
// scratch.grad[1], then the energy cotangents.
template <typename T>
static int trace_backward_begin(lynx_ctx* ctx, lynx_lattice* lat, const void* d_energy_in) {
  int rc;
  if ((rc = sync_pool(ctx, lat))) return rc;  // (k_build_bwd and k_trace_energy_bwd read the parameters from memory)
  if ((rc = trace_table<T>(ctx, lat, d_energy_in))) return rc;
  return ensure_tbar_scratch<T>(ctx, lat);
}

template <typename T>
static int trace_backward_finish(lynx_ctx* ctx, lynx_lattice* lat, const void* d_energy_in, const void* d_energy_bar,
                                 void* d_grad_params, void* d_grad_energy_in) {
  if (const int rc = launch_build_bwd<T>(ctx, lat, d_energy_in, d_grad_params, d_grad_energy_in, 0, false)) return rc;
  if (d_energy_bar) {
    hipLaunchKernelGGL(k_trace_energy_bwd<T>, dim3((unsigned)((lat->batch + 63) / 64)), dim3(64), 0, ctx->stream, dev_view(lat),
                       (const T*)ctx->scratch.steps[lynx_ctx::kTableTrace].buf, (const T*)d_energy_bar, (T*)d_grad_params,
                       (T*)d_grad_energy_in);
    HIP_TRY(ctx, hipGetLastError());
  }
  return LYNX_OK;
}

// the reverse sweep of the moment recursion with a cotangent at every point (k_trace_moments_bwd) -> T_bar
template <typename T, typename ST>
static int trace_backward_moments(lynx_ctx* ctx, lynx_lattice* lat, const void* d_mu_trace, const void* d_cov_trace,
                                  const void* d_mu_bar, const void* d_cov_bar, void* d_grad_mu_in, void* d_grad_cov_in) {
  hipLaunchKernelGGL((k_trace_moments_bwd<T, ST>), dim3((unsigned)lat->batch), dim3(64), 0, ctx->stream, (int)lat->n_steps,
                     (const T*)ctx->scratch.steps[lynx_ctx::kTableTrace].buf, (const ST*)d_mu_trace, (const ST*)d_cov_trace,
                     (const ST*)d_mu_bar, (const ST*)d_cov_bar, (T*)ctx->scratch.grad[1].buf, (T*)d_grad_mu_in, (T*)d_grad_cov_in);
  HIP_TRY(ctx, hipGetLastError());
  return LYNX_OK;
}

template <typename T, typename ST = T>
static int trace_backward_t(lynx_ctx* ctx, lynx_lattice* lat, const void* d_energy_in, const void* d_mu_trace,
                            const void* d_cov_trace, const void* d_mu_bar, const void* d_cov_bar, const void* d_energy_bar,
                            void* d_grad_params, void* d_grad_energy_in, void* d_grad_mu_in, void* d_grad_cov_in) {
  int rc;
  if ((rc = trace_backward_begin<T>(ctx, lat, d_energy_in))) return rc;
  if ((rc = trace_backward_moments<T, ST>(ctx, lat, d_mu_trace, d_cov_trace, d_mu_bar, d_cov_bar, d_grad_mu_in, d_grad_cov_in)))
    return rc;
  return trace_backward_finish<T>(ctx, lat, d_energy_in, d_energy_bar, d_grad_params, d_grad_energy_in);
}

// what every reverse entry point of the trace refuses about the lattice; `what`: the entry point's message prefix
static int trace_backward_check(lynx_ctx* ctx, lynx_lattice* lat, const std::string& what) {
  if (lat->n_steps <= 0) return fail(ctx, LYNX_ERR_INVALID, what + "empty program");
  if (lat->n_steps > kTraceBwdMaxSteps || lat->n_elems > kTraceBwdMaxSteps)
    return fail(ctx, LYNX_ERR_INVALID, what + "more than 256 elements");
  if (lat->batch <= 0 || lat->batch > 0x7fffffffLL) return fail(ctx, LYNX_ERR_INVALID, what + "bad batch");
  if ((int64_t)lat->batch * (lat->n_steps + 1) > 0x7fffffffLL)
    return fail(ctx, LYNX_ERR_INVALID, what + "batch x points too large for one launch");
  return LYNX_OK;
}

// The moments of a fixed set of particles are closed under affine maps only: behind a cavity's kick they are not a
// function of the moments in front of it.
static int trace_backward_no_cavity(lynx_ctx* ctx, lynx_lattice* lat, const std::string& what) {
  for (int32_t s = 0; s < lat->n_steps; ++s)
    if (lat->h_steps[s].kind == LYNX_STEP_CAVITY)
      return fail(ctx, LYNX_ERR_INVALID,
                  what + "step " + std::to_string(s) + " is a cavity step (the particles' moments are not closed under its kick)");
  return LYNX_OK;
}

int lynx_track_moments_along_backward(lynx_ctx* ctx, lynx_lattice* lat, const void* d_energy_in, const void* d_mu_trace,
                                      const void* d_cov_trace, const void* d_mu_bar, const void* d_cov_bar,
                                      const void* d_energy_bar, void* d_grad_params, void* d_grad_energy_in,
                                      void* d_grad_mu_in, void* d_grad_cov_in) {
  LYNX_MAIN_ENTRY(ctx);
  if (!lat || !d_energy_in || !d_mu_trace || !d_cov_trace || !d_mu_bar || !d_cov_bar || !d_grad_params ||
      !d_grad_energy_in || !d_grad_mu_in || !d_grad_cov_in)
    return fail(ctx, LYNX_ERR_INVALID, "null argument");
  if (const int rc = trace_backward_check(ctx, lat, "beam trace gradients: ")) return rc;
  LYNX_MAIN_WRITES(ctx, kFeedsBuild, reverse_writes(lat, d_grad_params, d_grad_energy_in, d_grad_mu_in, d_grad_cov_in));
  return with_dtype(lat->dtype, [&](auto zero) {
    return trace_backward_t<decltype(zero)>(ctx, lat, d_energy_in, d_mu_trace, d_cov_trace, d_mu_bar, d_cov_bar, d_energy_bar,
                                            d_grad_params, d_grad_energy_in, d_grad_mu_in, d_grad_cov_in);
  });
}

// A ParticleBeam's states and cotangents of the sweep in scratch.grad[0]: mu [7] | cov [49] | mu_bar [7] | cov_bar [49] per
// (sample, point), block by block, in the float64 of the records (k_trace_records_to_states), and `behind` more scalars
// behind them for the caller.  Null records: no moment sweep -- no blocks, no launch, `behind` starts the scratch.
struct TraceSweepStates {
  double *mu, *cov, *mu_bar, *cov_bar, *behind;
};
static int trace_sweep_states(lynx_ctx* ctx, lynx_lattice* lat, const double* d_trace_fwd, const double* d_grad_trace,
                              size_t behind, TraceSweepStates* st) {
  const int64_t points = lat->batch * ((int64_t)lat->n_steps + 1);
  const size_t state_scalars = d_trace_fwd ? (size_t)points * 112 : 0;
  int rc;
  if ((rc = ensure_scratch(ctx, ctx->scratch.grad[0], std::max<size_t>(state_scalars + behind, 1) * sizeof(double))))
    return rc;
  st->mu = (double*)ctx->scratch.grad[0].buf;
  st->cov = st->mu + points * 7;
  st->mu_bar = st->cov + points * 49;
  st->cov_bar = st->mu_bar + points * 7;
  st->behind = st->mu + state_scalars;
  if (!d_trace_fwd) return LYNX_OK;
  hipLaunchKernelGGL(k_trace_records_to_states, dim3((unsigned)points), dim3(64), 0, ctx->stream, d_trace_fwd, d_grad_trace,
                     st->mu, st->cov, st->mu_bar, st->cov_bar);
  HIP_TRY(ctx, hipGetLastError());
  return LYNX_OK;
}

template <typename T>
static int particles_along_backward_t(lynx_ctx* ctx, lynx_lattice* lat, const void* d_energy_in, const double* d_trace_fwd,
                                      const double* d_grad_trace, const void* d_energy_bar, void* d_grad_params,
                                      void* d_grad_energy_in, void* d_grad_mean_in, void* d_grad_cov_in) {
  TraceSweepStates st;
  if (const int rc = trace_sweep_states(ctx, lat, d_trace_fwd, d_grad_trace, 0, &st)) return rc;
  return trace_backward_t<T, double>(ctx, lat, d_energy_in, st.mu, st.cov, st.mu_bar, st.cov_bar, d_energy_bar, d_grad_params,
                                     d_grad_energy_in, d_grad_mean_in, d_grad_cov_in);
}

int lynx_track_particles_along_backward(lynx_ctx* ctx, lynx_lattice* lat, int64_t n_particles, const void* d_energy_in,
                                        const double* d_trace_fwd, const double* d_grad_trace, const void* d_energy_bar,
                                        void* d_grad_params, void* d_grad_energy_in, void* d_grad_mean_in,
                                        void* d_grad_cov_in) {
  LYNX_MAIN_ENTRY(ctx);
  if (!lat || !d_energy_in || !d_trace_fwd || !d_grad_trace || !d_grad_params || !d_grad_energy_in || !d_grad_mean_in ||
      !d_grad_cov_in)
    return fail(ctx, LYNX_ERR_INVALID, "null argument");
  if (n_particles <= 0) return fail(ctx, LYNX_ERR_INVALID, "n_particles must be > 0");
  if (const int rc = trace_backward_check(ctx, lat, "beam trace gradients: ")) return rc;
  if (const int rc = trace_backward_no_cavity(ctx, lat, "beam trace gradients of a ParticleBeam: ")) return rc;
  LYNX_MAIN_WRITES(ctx, kFeedsBuild, reverse_writes(lat, d_grad_params, d_grad_energy_in, d_grad_mean_in, d_grad_cov_in));
  return with_dtype(lat->dtype, [&](auto zero) {
    return particles_along_backward_t<decltype(zero)>(ctx, lat, d_energy_in, d_trace_fwd, d_grad_trace, d_energy_bar, d_grad_params,
                                                      d_grad_energy_in, d_grad_mean_in, d_grad_cov_in);
  });
}

// ---- forward-mode pass of the beam trace: tangents of the moments at every point -------------

// The directions of a forward-mode call as the host hands them over (CSR: dir_start [D + 1], the rest [n]).
struct TraceDirectionList {
  int32_t count, entries;
  const int32_t *start, *leaf, *row;
  const double* weight;
};

// Every refusal of the forward-mode entry points about the lattice and the directions, before anything is launched.
// `cavities`: the entry that walks through cavity steps -- they are no refusal, a voltage, phase or frequency on a cavity
// that is no step of its own is.
static int trace_forward_check(lynx_ctx* ctx, lynx_lattice* lat, const TraceDirectionList& dl, bool cavities = false) {
  const std::string what = "beam trace tangents: ";
  if (!dl.start || !dl.leaf || !dl.row || !dl.weight) return fail(ctx, LYNX_ERR_INVALID, what + "null argument");
  if (dl.count < 1) return fail(ctx, LYNX_ERR_INVALID, what + "n_directions must be > 0");
  if (dl.entries < 0) return fail(ctx, LYNX_ERR_INVALID, what + "n_entries must be >= 0");
  if (lat->n_steps <= 0) return fail(ctx, LYNX_ERR_INVALID, what + "empty program");
  if (lat->batch <= 0 || lat->batch > 0x7fffffffLL) return fail(ctx, LYNX_ERR_INVALID, what + "bad batch");
  for (int32_t s = 0; s < lat->n_steps; ++s) {
    const lynx_step& st = lat->h_steps[s];
    if (st.kind == LYNX_STEP_CAVITY && !cavities)
      return fail(ctx, LYNX_ERR_INVALID,
                  what + "step " + std::to_string(s) + " is a cavity step (the energy behind it, and with it every later map, depends on "
                         "its parameters, and the particles' moments are not closed under its kick)");
    if (st.first != s || st.last != s + 1 || lat->n_elems != lat->n_steps)
      return fail(ctx, LYNX_ERR_INVALID, what + "not the trace's program (every element a step of its own)");
  }
  if ((int64_t)lat->batch * (lat->n_steps + 1) > 0x7fffffffLL || (int64_t)lat->batch * dl.count > 0x7fffffffLL ||
      ((int64_t)lat->batch * dl.entries + 63) / 64 > 0x7fffffffLL)
    return fail(ctx, LYNX_ERR_INVALID, what + "batch x points, directions or entries too large for one launch");
  if (dl.start[0] != 0 || dl.start[dl.count] != dl.entries)
    return fail(ctx, LYNX_ERR_INVALID, what + "dir_start does not run from 0 to n_entries");
  for (int32_t d = 0; d < dl.count; ++d)
    if (dl.start[d + 1] < dl.start[d] || dl.start[d + 1] > dl.entries)
      return fail(ctx, LYNX_ERR_INVALID, what + "dir_start decreases at direction " + std::to_string(d));
  for (int32_t q = 0; q < dl.entries; ++q) {
    const std::string entry = "entry " + std::to_string(q);
    if (dl.leaf[q] < 0 || dl.leaf[q] >= lat->n_elems)
      return fail(ctx, LYNX_ERR_INVALID, what + entry + ": leaf " + std::to_string(dl.leaf[q]) + " out of range");
    if (dl.row[q] < 0 || dl.row[q] > kGradParams)
      return fail(ctx, LYNX_ERR_INVALID, what + entry + ": row " + std::to_string(dl.row[q]) + " out of range");
    const int kind = lat->h_elems[dl.leaf[q]].kind;
    if (dl.row[q] != kGradParams && dl.row[q] >= bwd_kind_params(kind))  // (the energy: every kind, zero for one without parameters)
      return fail(ctx, LYNX_ERR_INVALID,
                  what + entry + ": an element of kind " + std::to_string(kind) + " has no parameter row " + std::to_string(dl.row[q]));
    if (cavities && kind == LYNX_KIND_CAVITY && dl.row[q] >= 1 && dl.row[q] <= 3 && lat->h_steps[dl.leaf[q]].kind != LYNX_STEP_CAVITY)
      return fail(ctx, LYNX_ERR_INVALID,
                  what + entry + ": row " + std::to_string(dl.row[q]) + " of the cavity at leaf " + std::to_string(dl.leaf[q]) +
                      ", which is not a cavity step (without voltage its map has no continuous limit in voltage, phase or frequency)");
  }
  return LYNX_OK;
}

// Where a forward-mode call's scratch lies in scratch.trace_jvp: the directions, the entries' weight . dM, and (a
// ParticleBeam) the states of the sweep.
struct TraceForwardScratch {
  TraceDirections dirs;
  double *mdot, *mu, *cov;
  const double* seed;  // through cavities: the directions' energy seeds [D], behind the weights
  void* energy;        // ... and the energy that enters every step [B][P], lattice dtype
};

// The directions on the device, the entries of each direction ordered by leaf (stable: entries on one leaf keep their
// order) -- uploaded when they differ from what is there, like the trace's plan: the wait that upload needs is paid once
// per set of directions, and a loop that asks for the same tangents again pays nothing.
// `seed` (through cavities): the energy seeds ride behind the weights, an entry's tangent is 64 wide and the energies
// [B][P] follow.
static int trace_forward_scratch(lynx_ctx* ctx, lynx_lattice* lat, const TraceDirectionList& dl, bool states, TraceForwardScratch* out,
                                 const double* seed = nullptr) {
  const int32_t D = dl.count, n = dl.entries;
  const size_t ints = (size_t)D + 1 + 2 * (size_t)n;
  const size_t words = (ints + 1) / 2 * 2 + 2 * (size_t)n + (seed ? 2 * (size_t)D : 0);  // (the weights, the seeds: 8-aligned)
  std::vector<int32_t> plan(words, 0);
  int32_t* weights = plan.data() + (ints + 1) / 2 * 2;  // (two words each)
  std::vector<int32_t> order(std::max(n, 1));
  for (int32_t q = 0; q < n; ++q) order[q] = q;
  for (int32_t d = 0; d < D; ++d)
    std::stable_sort(order.begin() + dl.start[d], order.begin() + dl.start[d + 1],
                     [&](int32_t a, int32_t b) { return dl.leaf[a] < dl.leaf[b]; });
  for (int32_t d = 0; d <= D; ++d) plan[d] = dl.start[d];
  for (int32_t q = 0; q < n; ++q) {
    plan[(size_t)D + 1 + q] = dl.leaf[order[q]];
    plan[(size_t)D + 1 + n + q] = dl.row[order[q]];
    std::memcpy(weights + 2 * (size_t)q, dl.weight + order[q], sizeof(double));
  }
  if (seed) std::memcpy(weights + 2 * (size_t)n, seed, (size_t)D * sizeof(double));
  const int64_t points = lat->batch * ((int64_t)lat->n_steps + 1);
  const size_t plan_bytes = (words * sizeof(int32_t) + 255) / 256 * 256;
  const size_t mdot_scalars = std::max<size_t>((size_t)lat->batch * n * (seed ? LYNX_STEP_STRIDE : 49), 1);
  const size_t need = plan_bytes + (mdot_scalars + (states ? (size_t)points * 56 : 0) + (seed ? (size_t)points : 0)) * sizeof(double);
  Scratch& sc = ctx->scratch.trace_jvp;
  const bool fresh = sc.bytes < need;
  int rc;
  if ((rc = ensure_scratch(ctx, sc, need))) return rc;
  if (fresh || plan != ctx->trace_dirs) {
    ctx->trace_dirs.clear();
    HIP_TRY(ctx, hipMemcpyAsync(sc.buf, plan.data(), words * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, sync_main(ctx));  // (kernels of earlier calls have read the old directions; the host vector is ours again)
    ctx->trace_dirs.swap(plan);
  }
  const int32_t* base = (const int32_t*)sc.buf;
  out->dirs = TraceDirections{base, base + D + 1, base + D + 1 + n, (const double*)(base + (ints + 1) / 2 * 2), D, n};
  out->mdot = (double*)((char*)sc.buf + plan_bytes);
  out->mu = out->mdot + mdot_scalars;
  out->cov = out->mu + points * 7;
  out->seed = seed ? out->dirs.weight + n : nullptr;
  out->energy = seed ? out->mdot + mdot_scalars : nullptr;  // (no states with a seed: a ParameterBeam's entry)
  return LYNX_OK;
}

// k_trace_tangent_maps, then the sweep over the states `d_mu`, `d_cov` of type ST.
template <typename T, typename ST>
static int trace_forward_sweep(lynx_ctx* ctx, lynx_lattice* lat, const void* d_energy_in, const TraceForwardScratch& fs,
                               const void* d_mu, const void* d_cov, double* d_mu_dot, double* d_cov_dot) {
  const int64_t B = lat->batch, threads = B * fs.dirs.entries;
  if (threads > 0) {
    hipLaunchKernelGGL(k_trace_tangent_maps<T>, dim3((unsigned)((threads + 63) / 64)), dim3(64), 0, ctx->stream, dev_view(lat),
                       (const T*)d_energy_in, fs.dirs, fs.mdot);
    HIP_TRY(ctx, hipGetLastError());
  }
  hipLaunchKernelGGL((k_trace_moments_jvp<T, ST>), dim3((unsigned)(B * fs.dirs.count)), dim3(64), 0, ctx->stream, (int)lat->n_steps,
                     fs.dirs, (const T*)ctx->scratch.steps[lynx_ctx::kTableTrace].buf, (const ST*)d_mu, (const ST*)d_cov,
                     (const double*)fs.mdot, d_mu_dot, d_cov_dot);
  HIP_TRY(ctx, hipGetLastError());
  return LYNX_OK;
}

// what both entry points do in front of the sweep: the parameters in memory (k_trace_tangent_maps reads them there), the
// trace's table in the trace's own slot, the directions
template <typename T>
static int trace_forward_begin(lynx_ctx* ctx, lynx_lattice* lat, const void* d_energy_in, const TraceDirectionList& dl, bool states,
                               TraceForwardScratch* fs, const double* seed = nullptr) {
  int rc;
  if ((rc = sync_pool(ctx, lat))) return rc;
  if ((rc = trace_forward_scratch(ctx, lat, dl, states, fs, seed))) return rc;
  ctx->main_idle = false;  // (the upload of new directions has waited for the stream: work follows it now)
  return trace_table<T>(ctx, lat, d_energy_in);
}

static std::array<Written, 2> forward_writes(const lynx_lattice* lat, int32_t n_directions, double* d_mu_dot, double* d_cov_dot) {
  const size_t cells = (size_t)lat->batch * std::max(n_directions, 0) * ((size_t)lat->n_steps + 1);
  return {{{d_mu_dot, cells * 7 * sizeof(double)}, {d_cov_dot, cells * 49 * sizeof(double)}}};
}

int lynx_track_moments_along_forward(lynx_ctx* ctx, lynx_lattice* lat, const void* d_energy_in, const void* d_mu_trace,
                                     const void* d_cov_trace, const int32_t* dir_start, const int32_t* dir_leaf,
                                     const int32_t* dir_row, const double* dir_weight, int32_t n_directions, int32_t n_entries,
                                     double* d_mu_dot, double* d_cov_dot) {
  LYNX_MAIN_ENTRY(ctx);
  if (!lat || !d_energy_in || !d_mu_trace || !d_cov_trace || !d_mu_dot || !d_cov_dot)
    return fail(ctx, LYNX_ERR_INVALID, "beam trace tangents: null argument");
  const TraceDirectionList dl{n_directions, n_entries, dir_start, dir_leaf, dir_row, dir_weight};
  if (const int rc = trace_forward_check(ctx, lat, dl)) return rc;
  LYNX_MAIN_WRITES(ctx, kFeedsBuild, forward_writes(lat, n_directions, d_mu_dot, d_cov_dot));
  return with_dtype(lat->dtype, [&](auto zero) {
    using T = decltype(zero);
    TraceForwardScratch fs;
    if (const int rc = trace_forward_begin<T>(ctx, lat, d_energy_in, dl, false, &fs)) return rc;
    return trace_forward_sweep<T, T>(ctx, lat, d_energy_in, fs, d_mu_trace, d_cov_trace, d_mu_dot, d_cov_dot);
  });
}

int lynx_track_particles_along_forward(lynx_ctx* ctx, lynx_lattice* lat, int64_t n_particles, const void* d_energy_in,
                                       const double* d_trace_fwd, const int32_t* dir_start, const int32_t* dir_leaf,
                                       const int32_t* dir_row, const double* dir_weight, int32_t n_directions, int32_t n_entries,
                                       double* d_mu_dot, double* d_cov_dot) {
  LYNX_MAIN_ENTRY(ctx);
  if (!lat || !d_energy_in || !d_trace_fwd || !d_mu_dot || !d_cov_dot)
    return fail(ctx, LYNX_ERR_INVALID, "beam trace tangents: null argument");
  if (n_particles <= 0) return fail(ctx, LYNX_ERR_INVALID, "beam trace tangents: n_particles must be > 0");
  const TraceDirectionList dl{n_directions, n_entries, dir_start, dir_leaf, dir_row, dir_weight};
  if (const int rc = trace_forward_check(ctx, lat, dl)) return rc;
  LYNX_MAIN_WRITES(ctx, kFeedsBuild, forward_writes(lat, n_directions, d_mu_dot, d_cov_dot));
  return with_dtype(lat->dtype, [&](auto zero) {
    using T = decltype(zero);
    TraceForwardScratch fs;
    if (const int rc = trace_forward_begin<T>(ctx, lat, d_energy_in, dl, true, &fs)) return rc;
    const int64_t points = lat->batch * ((int64_t)lat->n_steps + 1);
    hipLaunchKernelGGL(k_trace_records_to_moments, dim3((unsigned)points), dim3(64), 0, ctx->stream, d_trace_fwd, fs.mu, fs.cov);
    HIP_TRY(ctx, hipGetLastError());
    return trace_forward_sweep<T, double>(ctx, lat, d_energy_in, fs, fs.mu, fs.cov, d_mu_dot, d_cov_dot);
  });
}

// ... through cavity steps (a ParameterBeam): the energy that enters every step and its tangent along every direction,
// the entries' tangent rows at those energies, the sweep with the cavity branch's tangent (lynx_trace_jvp.hpp).
template <typename T>
static int trace_forward_sweep_cavities(lynx_ctx* ctx, lynx_lattice* lat, const void* d_energy_in, const TraceForwardScratch& fs,
                                        const void* d_mu, const void* d_cov, double* d_mu_dot, double* d_cov_dot, double* d_energy_dot) {
  const int64_t B = lat->batch, pairs = B * fs.dirs.count, threads = B * fs.dirs.entries;
  const T* table = (const T*)ctx->scratch.steps[lynx_ctx::kTableTrace].buf;
  hipLaunchKernelGGL(k_trace_energies<T>, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, ctx->stream, dev_view(lat), table,
                     (const T*)d_energy_in, (T*)fs.energy);
  HIP_TRY(ctx, hipGetLastError());
  hipLaunchKernelGGL(k_trace_energy_tangents<T>, dim3((unsigned)((pairs + 63) / 64)), dim3(64), 0, ctx->stream, dev_view(lat), table,
                     fs.dirs, fs.seed, d_energy_dot);
  HIP_TRY(ctx, hipGetLastError());
  if (threads > 0) {
    hipLaunchKernelGGL(k_trace_tangent_rows<T>, dim3((unsigned)((threads + 63) / 64)), dim3(64), 0, ctx->stream, dev_view(lat),
                       (const T*)fs.energy, fs.dirs, (const double*)d_energy_dot, fs.mdot);
    HIP_TRY(ctx, hipGetLastError());
  }
  hipLaunchKernelGGL(k_trace_moments_jvp_kicks<T>, dim3((unsigned)pairs), dim3(64), 0, ctx->stream, (int)lat->n_steps, fs.dirs, table,
                     (const T*)d_mu, (const T*)d_cov, (const double*)fs.mdot, d_mu_dot, d_cov_dot);
  HIP_TRY(ctx, hipGetLastError());
  return LYNX_OK;
}

int lynx_track_moments_along_forward_cavities(lynx_ctx* ctx, lynx_lattice* lat, const void* d_energy_in, const void* d_mu_trace,
                                              const void* d_cov_trace, const int32_t* dir_start, const int32_t* dir_leaf,
                                              const int32_t* dir_row, const double* dir_weight, int32_t n_directions,
                                              int32_t n_entries, double* d_mu_dot, double* d_cov_dot,
                                              const double* dir_energy_seed, double* d_energy_dot) {
  LYNX_MAIN_ENTRY(ctx);
  if (!lat || !d_energy_in || !d_mu_trace || !d_cov_trace || !d_mu_dot || !d_cov_dot || !dir_energy_seed || !d_energy_dot)
    return fail(ctx, LYNX_ERR_INVALID, "beam trace tangents: null argument");
  const TraceDirectionList dl{n_directions, n_entries, dir_start, dir_leaf, dir_row, dir_weight};
  if (const int rc = trace_forward_check(ctx, lat, dl, true)) return rc;
  const auto two = forward_writes(lat, n_directions, d_mu_dot, d_cov_dot);
  LYNX_MAIN_WRITES(ctx, kFeedsBuild, {two[0], two[1], {d_energy_dot, two[0].bytes / 7}});
  return with_dtype(lat->dtype, [&](auto zero) {
    using T = decltype(zero);
    TraceForwardScratch fs;
    if (const int rc = trace_forward_begin<T>(ctx, lat, d_energy_in, dl, false, &fs, dir_energy_seed)) return rc;
    return trace_forward_sweep_cavities<T>(ctx, lat, d_energy_in, fs, d_mu_trace, d_cov_trace, d_mu_dot, d_cov_dot, d_energy_dot);
  });
}

// ... through cavity steps: k_track_bwd's sweep over the particles with a moment cotangent injected at every point
// (k_track_bwd_inject), on the trace's program -- every step a unit of its own --, its partial sums reduced into
// scratch.grad[1] as track_backward_t reduces them, then the same k_build_bwd.  scratch.grad[0]: the partial sums
// [B][chunks][S][64], then the injection table [B][P][kInjectStride], both in the lattice's dtype.
template <typename T, typename Z>
static int particles_along_backward_cavities_t(lynx_ctx* ctx, lynx_lattice* lat, int64_t N, const void* d_energy_in,
                                               const void* d_p_in, int flags, const double* d_trace_fwd,
                                               const double* d_grad_trace, const void* d_energy_bar, void* d_grad_params,
                                               void* d_grad_energy_in, void* d_grad_p_in) {
  constexpr int W = LaneOf<Z>::W;
  const int64_t B = lat->batch;
  const int32_t S = lat->n_steps, P = S + 1;
  int rc;
  BwdArgs a;
  (void)plan_bwd_units(lat, false, false, &a);  // (the entry point has refused more steps than the sweep parks)
  const BwdSweepPlan p = plan_bwd_sweep<T, W>(ctx, B, N, S, &a);
  a.n_work = (int32_t)(B * p.chunks);
  if ((int64_t)B * p.chunks > 0x7fffffffLL) return fail(ctx, LYNX_ERR_INVALID, "beam trace gradients with cavities: grid too large");
  if ((rc = allow_lds(ctx, k_track_bwd_inject<T, Z>, p.lds))) return rc;
  // (sized before trace_backward_begin, the table launched behind it: what is refused is refused before the build)
  const size_t partial_scalars = (size_t)B * p.chunks * S * kGradStride, table_scalars = (size_t)B * P * kInjectStride;
  if ((rc = ensure_scratch(ctx, ctx->scratch.grad[0], (partial_scalars + table_scalars) * sizeof(T))))
    return rc;
  T* partials = (T*)ctx->scratch.grad[0].buf;
  T* inject = partials + partial_scalars;
  if ((rc = trace_backward_begin<T>(ctx, lat, d_energy_in))) return rc;
  hipLaunchKernelGGL(k_trace_inject_table<T>, dim3((unsigned)((table_scalars + 255) / 256)), dim3(256), 0, ctx->stream, d_trace_fwd,
                     d_grad_trace, (int64_t)table_scalars, inject);
  HIP_TRY(ctx, hipGetLastError());
  // (between lynx_profile_begin and _end the sweep's own duration is one more entry of lynx_profile_launches)
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (ctx->profiling) {
    HIP_TRY(ctx, hipEventCreateWithFlags(&e0, timing_event_flags(ctx)));
    HIP_TRY(ctx, hipEventCreateWithFlags(&e1, timing_event_flags(ctx)));
  }
  hipExtLaunchKernelGGL((k_track_bwd_inject<T, Z>), dim3((unsigned)(B * p.chunks)), dim3(kTrackThreads), (std::uint32_t)p.lds, ctx->stream,
                        e0, e1, 0u, dev_view(lat), a, (const T*)d_p_in, (flags & LYNX_TRACK_SHARED_INPUT) ? (int64_t)0 : N * 7,
                        (const T*)ctx->scratch.steps[lynx_ctx::kTableTrace].buf, (const T*)inject, partials, (T*)d_grad_p_in);
  HIP_TRY(ctx, hipGetLastError());
  if (ctx->profiling) ctx->prof_events.emplace_back(e0, e1);
  if ((rc = reduce_tbar<T>(ctx, partials, B, S, p.chunks))) return rc;
  return trace_backward_finish<T>(ctx, lat, d_energy_in, d_energy_bar, d_grad_params, d_grad_energy_in);
}

int lynx_track_particles_along_backward_cavities(lynx_ctx* ctx, lynx_lattice* lat, int64_t n_particles,
                                                 const void* d_energy_in, const void* d_p_in, int flags,
                                                 const double* d_trace_fwd, const double* d_grad_trace,
                                                 const void* d_energy_bar, void* d_grad_params, void* d_grad_energy_in,
                                                 void* d_grad_p_in) {
  LYNX_MAIN_ENTRY(ctx);
  const std::string prefix = "beam trace gradients with cavities: ";
  const auto refuse = [&](const std::string& what) { return fail(ctx, LYNX_ERR_INVALID, prefix + what); };
  if (!lat || !d_energy_in || !d_p_in || !d_trace_fwd || !d_grad_trace || !d_grad_params || !d_grad_energy_in)
    return refuse("null argument");
  if (n_particles < 1) return refuse("n_particles must be > 0");
  if (flags & ~LYNX_TRACK_SHARED_INPUT) return refuse("LYNX_TRACK_SHARED_INPUT is the only flag");
  if (const int rc = trace_backward_check(ctx, lat, prefix)) return rc;
  if (lat->n_steps > kBwdGroup * kBwdMaxGroups)
    return refuse(std::to_string(lat->n_steps) + " steps; the sweep over the particles parks at most " +
                  std::to_string(kBwdGroup * kBwdMaxGroups) + " (split the lattice)");
  const size_t lds = lat->dtype == LYNX_F64 ? bwd_stream_lds_bytes<double, 1>(lat->n_steps) : bwd_stream_lds_bytes<float, 2>(lat->n_steps);
  if (const int rc = refuse_bwd_stream_lds(ctx, prefix.c_str(), lat->n_steps, lds)) return rc;
  if (d_grad_p_in && d_grad_p_in == d_p_in) return refuse("d_grad_p_in aliases d_p_in: the sweep reads the incoming particles tile by tile");
  LYNX_MAIN_WRITES(ctx, kFeedsBuild, reverse_writes(lat, d_grad_params, d_grad_energy_in, nullptr, nullptr,
                                                    {d_grad_p_in, (size_t)lat->batch * n_particles * 7 * dtype_size(lat->dtype)}));
  const auto pass = lat->dtype == LYNX_F64 ? particles_along_backward_cavities_t<double, double>
                                           : particles_along_backward_cavities_t<float, lynx_f32x2>;
  return pass(ctx, lat, n_particles, d_energy_in, d_p_in, flags, d_trace_fwd, d_grad_trace, d_energy_bar, d_grad_params,
              d_grad_energy_in, d_grad_p_in);
}

// ... of a trace with losses: one wave per (sample, survivor set) propagates the set's incoming moments and sweeps back
// over the set's live points (k_trace_moments_bwd_sets), the sets' T_bar are added in set order (k_trace_sum_sets), then
// the same k_build_bwd.  scratch.grad[0]: the states [B][A + 1][S][56], then the sets' T_bar [A + 1][B][S][64], float64.
template <typename T>
static int particles_along_backward_losses_t(lynx_ctx* ctx, lynx_lattice* lat, const void* d_energy_in, const double* d_grad_trace,
                                             const void* d_energy_bar, const TraceLossSets& sets, const double* d_set_records,
                                             void* d_grad_params, void* d_grad_energy_in) {
  const int64_t B = lat->batch, S = lat->n_steps, J = sets.sets;
  const size_t state_scalars = (size_t)B * J * S * kSetState, tbar_scalars = (size_t)J * B * S * kGradStride;
  int rc;
  if ((rc = ensure_scratch(ctx, ctx->scratch.grad[0], (state_scalars + tbar_scalars) * sizeof(double))))
    return rc;
  double* states = (double*)ctx->scratch.grad[0].buf;
  double* tbar_sets = states + state_scalars;
  if ((rc = trace_backward_begin<T>(ctx, lat, d_energy_in))) return rc;
  hipLaunchKernelGGL(k_trace_moments_bwd_sets<T>, dim3((unsigned)(B * J)), dim3(64), 0, ctx->stream, (int)S, B, sets,
                     (const T*)ctx->scratch.steps[lynx_ctx::kTableTrace].buf, d_set_records, d_grad_trace, states, tbar_sets);
  HIP_TRY(ctx, hipGetLastError());
  const int64_t cells = B * S * kGradStride;
  hipLaunchKernelGGL(k_trace_sum_sets<T>, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, ctx->stream, (const double*)tbar_sets,
                     (int)J, cells, (T*)ctx->scratch.grad[1].buf);
  HIP_TRY(ctx, hipGetLastError());
  return trace_backward_finish<T>(ctx, lat, d_energy_in, d_energy_bar, d_grad_params, d_grad_energy_in);
}

int lynx_track_particles_along_backward_losses(lynx_ctx* ctx, lynx_lattice* lat, int64_t n_particles, const void* d_energy_in,
                                               const double* d_trace_fwd, const double* d_grad_trace, const void* d_energy_bar,
                                               int32_t n_apertures, const int32_t* apertures, const double* d_set_records,
                                               void* d_grad_params, void* d_grad_energy_in) {
  LYNX_MAIN_ENTRY(ctx);
  const std::string prefix = "beam trace gradients with losses: ";
  const auto refuse = [&](const std::string& what) { return fail(ctx, LYNX_ERR_INVALID, prefix + what); };
  if (!lat || !d_energy_in || !d_trace_fwd || !d_grad_trace || !apertures || !d_set_records || !d_grad_params || !d_grad_energy_in)
    return refuse("null argument");
  if (n_particles <= 0) return refuse("n_particles must be > 0");
  if (const int rc = trace_backward_check(ctx, lat, prefix)) return rc;
  if (n_apertures < 1 || n_apertures > kTraceMaxLossApertures)
    return refuse("n_apertures = " + std::to_string(n_apertures) + ", not 1 .. " + std::to_string(kTraceMaxLossApertures));
  if ((int64_t)lat->batch * (lat->n_steps + 1) * (n_apertures + 1) > 0x7fffffffLL)
    return refuse("batch x points x sets too large for one launch");
  if (const int rc = trace_backward_no_cavity(ctx, lat, prefix)) return rc;
  TraceLossSets sets{};
  sets.sets = n_apertures + 1;
  for (int32_t k = 0; k < n_apertures; ++k) {
    const int32_t step = apertures[k];
    if (step < 0 || step >= lat->n_steps || (k > 0 && step <= apertures[k - 1]))
      return refuse("aperture steps must be increasing and inside the program");
    const lynx_step& st = lat->h_steps[step];
    if (st.kind != LYNX_STEP_RUN || st.last != st.first + 1 || lat->h_elems[st.first].kind != LYNX_KIND_IDENTITY)
      return refuse("step " + std::to_string(step) + " is not an identity step: an aperture leaves the particles it passes alone");
    sets.last[k] = step;
  }
  sets.last[n_apertures] = lat->n_steps;
  LYNX_MAIN_WRITES(ctx, kFeedsBuild, reverse_writes(lat, d_grad_params, d_grad_energy_in, nullptr, nullptr));
  return with_dtype(lat->dtype, [&](auto zero) {
    return particles_along_backward_losses_t<decltype(zero)>(ctx, lat, d_energy_in, d_grad_trace, d_energy_bar, sets, d_set_records,
                                                             d_grad_params, d_grad_energy_in);
  });
}

// ... with the trajectories of chosen particles: k_trace_trajectories_bwd behind the moment sweep (or alone), then the
// same k_build_bwd.  scratch.grad[0]: the states of the moment sweep (if there is one), then the float64 row sums a
// sample's wave carries from tile to tile (if the chosen particles span several tiles).
template <typename T>
static int particles_along_backward_trajectories_t(lynx_ctx* ctx, lynx_lattice* lat, const void* d_energy_in,
                                                   const double* d_trace_fwd, const double* d_grad_trace, const void* d_energy_bar,
                                                   void* d_grad_params, void* d_grad_energy_in, void* d_grad_mean_in,
                                                   void* d_grad_cov_in, int64_t n_chosen, const void* d_trajectories,
                                                   const double* d_trajectories_bar, void* d_grad_chosen_in) {
  const int64_t B = lat->batch, S = lat->n_steps;
  const bool moments = d_trace_fwd != nullptr;
  const bool tiled = n_chosen > 64 * kChosenBwdSlots;
  int rc;
  TraceSweepStates st;
  if ((rc = trace_sweep_states(ctx, lat, d_trace_fwd, d_grad_trace, tiled ? (size_t)B * S * kGradStride : 0, &st))) return rc;
  double* partial = tiled ? st.behind : nullptr;
  if ((rc = trace_backward_begin<T>(ctx, lat, d_energy_in))) return rc;
  if (moments &&
      (rc = trace_backward_moments<T, double>(ctx, lat, st.mu, st.cov, st.mu_bar, st.cov_bar, d_grad_mean_in, d_grad_cov_in)))
    return rc;
  hipLaunchKernelGGL(k_trace_trajectories_bwd<T>, dim3((unsigned)B), dim3(64), 0, ctx->stream, (int)S, n_chosen,
                     (const T*)ctx->scratch.steps[lynx_ctx::kTableTrace].buf, (const T*)d_trajectories, d_trajectories_bar,
                     (T*)ctx->scratch.grad[1].buf, partial, moments ? 1 : 0, (T*)d_grad_chosen_in);
  HIP_TRY(ctx, hipGetLastError());
  return trace_backward_finish<T>(ctx, lat, d_energy_in, d_energy_bar, d_grad_params, d_grad_energy_in);
}

int lynx_track_particles_along_backward_trajectories(lynx_ctx* ctx, lynx_lattice* lat, int64_t n_particles,
                                                     const void* d_energy_in, const double* d_trace_fwd,
                                                     const double* d_grad_trace, const void* d_energy_bar, void* d_grad_params,
                                                     void* d_grad_energy_in, void* d_grad_mean_in, void* d_grad_cov_in,
                                                     int64_t n_chosen, const void* d_trajectories,
                                                     const double* d_trajectories_bar, void* d_grad_chosen_in) {
  LYNX_MAIN_ENTRY(ctx);
  const std::string what = "beam trace gradients with trajectories: ";
  if (!lat || !d_energy_in || !d_grad_params || !d_grad_energy_in || !d_trajectories || !d_trajectories_bar || !d_grad_chosen_in)
    return fail(ctx, LYNX_ERR_INVALID, what + "null argument");
  const int given = (d_trace_fwd != nullptr) + (d_grad_trace != nullptr) + (d_grad_mean_in != nullptr) + (d_grad_cov_in != nullptr);
  if (given != 0 && given != 4)
    return fail(ctx, LYNX_ERR_INVALID,
                what + "d_trace_fwd, d_grad_trace, d_grad_mean_in and d_grad_cov_in are given together or not at all");
  if (n_particles <= 0) return fail(ctx, LYNX_ERR_INVALID, what + "n_particles must be > 0");
  if (n_chosen <= 0) return fail(ctx, LYNX_ERR_INVALID, what + "n_chosen must be > 0");
  if (const int rc = trace_backward_check(ctx, lat, what)) return rc;
  // (a single trajectory is differentiable through the kick; a moment cotangent does not pass it)
  if (given)
    if (const int rc = trace_backward_no_cavity(ctx, lat, what)) return rc;
  LYNX_MAIN_WRITES(ctx, kFeedsBuild, reverse_writes(lat, d_grad_params, d_grad_energy_in, d_grad_mean_in, d_grad_cov_in,
                                                    {d_grad_chosen_in, (size_t)lat->batch * n_chosen * 7 * dtype_size(lat->dtype)}));
  return with_dtype(lat->dtype, [&](auto zero) {
    return particles_along_backward_trajectories_t<decltype(zero)>(ctx, lat, d_energy_in, d_trace_fwd, d_grad_trace, d_energy_bar,
                                                                   d_grad_params, d_grad_energy_in, d_grad_mean_in, d_grad_cov_in,
                                                                   n_chosen, d_trajectories, d_trajectories_bar, d_grad_chosen_in);
  });
}

// ---- screen read-out -------------------------------------------------------------------------

int lynx_histogram2d(lynx_ctx* ctx, int dtype, int64_t batch, int64_t n_particles, const void* d_p,
                     const void* d_xedges, const void* d_yedges, int32_t nx, int32_t ny, int32_t* d_image) {
  LYNX_MAIN_ENTRY(ctx);
  if (!d_p || !d_xedges || !d_yedges || !d_image || batch <= 0 || n_particles <= 0 || nx <= 0 || ny <= 0)
    return fail(ctx, LYNX_ERR_INVALID, "bad argument");
  const size_t lds = ((size_t)nx + ny + 2) * dtype_size(dtype);
  if (lds > 64 * 1024) return fail(ctx, LYNX_ERR_INVALID, "screen resolution too large for the edge table");
  LYNX_MAIN_WRITES(ctx, kFeedsNoBuild, {{d_image, (size_t)batch * nx * ny * sizeof(int32_t)}});
  HIP_TRY(ctx, hipMemsetAsync(d_image, 0, (size_t)batch * nx * ny * sizeof(int32_t), ctx->stream));
  const int64_t cus = compute_units(ctx);
  int64_t chunks = std::max<int64_t>(1, std::min<int64_t>((n_particles + 1023) / 1024, (8 * cus + batch - 1) / batch));
  if (batch * chunks > 0x7fffffffLL) return fail(ctx, LYNX_ERR_INVALID, "grid too large");
  with_dtype(dtype, [&](auto zero) {
    using T = decltype(zero);
    hipLaunchKernelGGL(k_histogram2d<T>, dim3((unsigned)(batch * chunks)), dim3(256), lds, ctx->stream, (const T*)d_p, n_particles,
                       (int)chunks, (const T*)d_xedges, (const T*)d_yedges, nx, ny, d_image);
  });
  HIP_TRY(ctx, hipGetLastError());
  return LYNX_OK;
}

int lynx_diag_phase_trig(lynx_ctx* ctx, int64_t n, const float* d_x, int32_t packed, float* d_sin, float* d_cos) {
  LYNX_MAIN_ENTRY(ctx);
  if (!d_x || !d_sin || !d_cos || n <= 0) return fail(ctx, LYNX_ERR_INVALID, "bad argument");
  LYNX_MAIN_WRITES(ctx, kFeedsNoBuild, {{d_sin, (size_t)n * sizeof(float)}, {d_cos, (size_t)n * sizeof(float)}});
  const int64_t threads = (n + 1) / 2;
  hipLaunchKernelGGL(k_diag_phase_trig, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, ctx->stream, d_x, n,
                     (int)packed, d_sin, d_cos);
  HIP_TRY(ctx, hipGetLastError());
  return LYNX_OK;
}

// ---- aperture ----------------------------------------------------------------------------

int lynx_aperture_mask(lynx_ctx* ctx, int dtype, int64_t batch, int64_t n_particles, const void* d_p,
                       const void* d_x_max, const void* d_y_max, int32_t param_stride, int32_t elliptical,
                       unsigned char* d_mask, int32_t* d_counts, int64_t* d_offsets, int64_t* d_totals) {
  LYNX_MAIN_ENTRY(ctx);
  if (!d_p || !d_x_max || !d_y_max || !d_mask || !d_counts || !d_offsets || !d_totals || batch <= 0 ||
      n_particles <= 0 || (param_stride != 0 && param_stride != 1))
    return fail(ctx, LYNX_ERR_INVALID, "bad argument");
  const int64_t chunks = (n_particles + kApertureChunk - 1) / kApertureChunk;
  if (batch * chunks > 0x7fffffffLL) return fail(ctx, LYNX_ERR_INVALID, "grid too large");
  LYNX_MAIN_WRITES(ctx, kFeedsNoBuild, {{d_mask, (size_t)batch * n_particles},
                                        {d_counts, (size_t)batch * chunks * sizeof(int32_t)},
                                        {d_offsets, (size_t)batch * chunks * sizeof(int64_t)},
                                        {d_totals, (size_t)batch * sizeof(int64_t)}});
  with_dtype(dtype, [&](auto zero) {
    using T = decltype(zero);
    hipLaunchKernelGGL(k_aperture_mask<T>, dim3((unsigned)(batch * chunks)), dim3(256), 0, ctx->stream, (const T*)d_p, n_particles,
                       (int)chunks, (const T*)d_x_max, (const T*)d_y_max, (int)param_stride, (int)elliptical, d_mask, d_counts);
  });
  HIP_TRY(ctx, hipGetLastError());
  hipLaunchKernelGGL(k_aperture_scan, dim3((unsigned)batch), dim3(256), 0, ctx->stream, d_counts, (int)chunks, d_offsets,
                     d_totals);
  HIP_TRY(ctx, hipGetLastError());
  return LYNX_OK;
}

int lynx_aperture_compact(lynx_ctx* ctx, int dtype, int64_t n_particles, const void* d_p, const unsigned char* d_mask,
                          const int64_t* d_offsets, void* d_kept, void* d_lost) {
  LYNX_MAIN_ENTRY(ctx);
  if (!d_p || !d_mask || !d_offsets || !d_kept || !d_lost || n_particles <= 0)
    return fail(ctx, LYNX_ERR_INVALID, "bad argument");
  const size_t bytes = (size_t)n_particles * 7 * dtype_size(dtype);
  LYNX_MAIN_WRITES(ctx, kFeedsNoBuild, {{d_kept, bytes}, {d_lost, bytes}});
  const int64_t chunks = (n_particles + kApertureChunk - 1) / kApertureChunk;
  with_dtype(dtype, [&](auto zero) {
    using T = decltype(zero);
    hipLaunchKernelGGL(k_aperture_compact<T>, dim3((unsigned)chunks), dim3(256), 0, ctx->stream, (const T*)d_p, n_particles, d_mask,
                       d_offsets, (T*)d_kept, (T*)d_lost);
  });
  HIP_TRY(ctx, hipGetLastError());
  return LYNX_OK;
}

int lynx_gaussian_image(lynx_ctx* ctx, int dtype, int64_t batch, const void* d_mu, const void* d_cov,
                        const void* d_xs, const void* d_ys, int32_t nx, int32_t ny, void* d_image) {
  LYNX_MAIN_ENTRY(ctx);
  if (!d_mu || !d_cov || !d_xs || !d_ys || !d_image || batch <= 0 || nx <= 0 || ny <= 0 || batch > 65535)
    return fail(ctx, LYNX_ERR_INVALID, "bad argument");
  LYNX_MAIN_WRITES(ctx, kFeedsNoBuild, {{d_image, (size_t)batch * nx * ny * dtype_size(dtype)}});
  const unsigned gx = (unsigned)(((int64_t)nx * ny + 255) / 256);
  with_dtype(dtype, [&](auto zero) {
    using T = decltype(zero);
    hipLaunchKernelGGL(k_gaussian_image<T>, dim3(gx, (unsigned)batch), dim3(256), 0, ctx->stream, (const T*)d_mu, (const T*)d_cov,
                       (const T*)d_xs, (const T*)d_ys, nx, ny, (T*)d_image);
  });
  HIP_TRY(ctx, hipGetLastError());
  return LYNX_OK;
}

// ---- the screen images of a ParameterBeam along a trace, their gradients and the image loss ----

// A screen of the caller's rows [n_screens][3] (point, nx, ny), with where its part of every per-screen array begins.
struct ImageScreen {
  int32_t point, nx, ny;
  int64_t cells;   // nx ny
  int64_t grid;    // its pixel positions in d_grid (xs, then ys)
  int64_t cell;    // its cells in a sample's images
  int64_t chunks;  // workgroups of kImageGradCells cells
  int64_t chunk;   // its chunks among all screens'
};
struct ImageScreens {
  std::vector<ImageScreen> rows;
  int64_t cells = 0, chunks = 0;  // of all screens
};

// What differs between the four entries' checks: the prefix of every refusal, what a bad argument is called, whether the
// dtype and the misalignments' stride are checked, and whether a screen is held to the 32 bits the sum kernels count its
// cells in.
struct ImageEntryChecks {
  const char* prefix;
  const char* bad_argument;
  bool dtype, stride, cell_limit;
};
constexpr ImageEntryChecks kImagesAlong{"images along the trace", "bad argument", false, true, false};
constexpr ImageEntryChecks kImageGradients{"image gradients along the trace", "image gradients along the trace: bad argument", true, true, true};
constexpr ImageEntryChecks kImageLoss{"image loss along the trace", "image loss along the trace: bad argument", true, true, true};
constexpr ImageEntryChecks kImageLossBackward{"image loss along the trace", "image loss along the trace: bad argument", true, false, true};

// The checks the four entries share, in the order they all make them (`given`: every pointer the entry needs is there),
// and the one walk over the caller's rows -> `list`.
static int image_screens(lynx_ctx* ctx, const ImageEntryChecks& entry, bool given, int dtype, int64_t batch, int32_t n_points,
                         int32_t n_screens, const int32_t* screens, int64_t misalignment_stride, ImageScreens* list) {
  const auto refuse = [&](const char* what) { return fail(ctx, LYNX_ERR_INVALID, std::string(entry.prefix) + ": " + what); };
  if (!given || !screens || batch <= 0 || batch > 65535 || n_points <= 0 || n_screens <= 0)
    return fail(ctx, LYNX_ERR_INVALID, entry.bad_argument);
  if (entry.dtype && dtype != LYNX_F32 && dtype != LYNX_F64) return refuse("the dtype is float32 or float64");
  if (entry.stride && misalignment_stride != 0 && misalignment_stride != 2 * (int64_t)n_screens)
    return refuse("the misalignments' sample stride is 0 or 2 * n_screens");
  int64_t grid = 0;
  for (int32_t k = 0; k < n_screens; ++k) {
    const int32_t point = screens[3 * k], nx = screens[3 * k + 1], ny = screens[3 * k + 2];
    if (point < 0 || point >= n_points || nx < 1 || ny < 1) return refuse("a screen's point lies inside the trace, and it has pixels");
    const int64_t cells = (int64_t)nx * ny, chunks = (cells + kImageGradCells - 1) / kImageGradCells;
    if (entry.cell_limit && cells > 0x7fffffffLL - kImageGradCells)  // (the kernel counts a screen's cells in 32 bits)
      return refuse("a screen has fewer than 2^31 - 2048 pixels");
    list->rows.push_back({point, nx, ny, cells, grid, list->cells, chunks, list->chunks});
    grid += (int64_t)nx + ny;
    list->cells += cells;
    list->chunks += chunks;
  }
  return LYNX_OK;
}

int lynx_gaussian_images_along(lynx_ctx* ctx, int dtype, int64_t batch, int32_t n_points, const void* d_mu_trace,
                               const void* d_cov_trace, int32_t n_screens, const int32_t* screens, const void* d_grid,
                               const void* d_misalignment, int64_t misalignment_stride, void* d_images) {
  LYNX_MAIN_ENTRY(ctx);
  ImageScreens list;
  if (const int rc = image_screens(ctx, kImagesAlong, d_mu_trace && d_cov_trace && d_grid && d_misalignment && d_images, dtype, batch,
                                   n_points, n_screens, screens, misalignment_stride, &list))
    return rc;
  LYNX_MAIN_WRITES(ctx, kFeedsBuild, {{d_images, (size_t)batch * list.cells * dtype_size(dtype)}});
  for (int32_t k = 0; k < n_screens; ++k) {
    const ImageScreen& s = list.rows[k];
    with_dtype(dtype, [&](auto zero) {
      using T = decltype(zero);
      hipLaunchKernelGGL(k_gaussian_image_along<T>, dim3((unsigned)((s.cells + 255) / 256), (unsigned)batch), dim3(256), 0, ctx->stream,
                         (const T*)d_mu_trace, (const T*)d_cov_trace, (int)n_points, (int)s.point, (const T*)d_grid + s.grid,
                         (const T*)d_grid + s.grid + s.nx, (int)s.nx, (int)s.ny, (const T*)d_misalignment + 2 * k, misalignment_stride,
                         (T*)d_images + s.cell, list.cells);
    });
    HIP_TRY(ctx, hipGetLastError());
  }
  return LYNX_OK;
}

int lynx_gaussian_images_along_backward(lynx_ctx* ctx, int dtype, int64_t batch, int32_t n_points, const void* d_mu_trace,
                                        const void* d_cov_trace, int32_t n_screens, const int32_t* screens, const void* d_grid,
                                        const void* d_misalignment, int64_t misalignment_stride, const void* d_images_bar,
                                        void* d_mu_bar, void* d_cov_bar, void* d_grad_misalignment) {
  LYNX_MAIN_ENTRY(ctx);
  ImageScreens list;
  if (const int rc = image_screens(ctx, kImageGradients,
                                   d_mu_trace && d_cov_trace && d_grid && d_misalignment && d_images_bar && d_mu_bar && d_cov_bar, dtype,
                                   batch, n_points, n_screens, screens, misalignment_stride, &list))
    return rc;
  const size_t es = dtype_size(dtype);
  LYNX_MAIN_WRITES(ctx, kFeedsBuild, {{d_mu_bar, (size_t)batch * n_points * 7 * es},
                                      {d_cov_bar, (size_t)batch * n_points * 49 * es},
                                      {d_grad_misalignment, (size_t)batch * n_screens * 2 * es}});
  // (every screen its own slab [B][chunks][6], screen after screen)
  if (const int rc = ensure_scratch(ctx, ctx->scratch.image_grad, (size_t)(batch * list.chunks * 6) * sizeof(double))) return rc;
  return with_dtype(dtype, [&](auto zero) {
    using T = decltype(zero);
    for (int32_t k = 0; k < n_screens; ++k) {
      const ImageScreen& s = list.rows[k];
      double* d_slab = (double*)ctx->scratch.image_grad.buf + batch * s.chunk * 6;
      hipLaunchKernelGGL(k_gaussian_image_along_bwd<T>, dim3((unsigned)s.chunks, (unsigned)batch), dim3(kImageGradThreads), 0,
                         ctx->stream, (const T*)d_mu_trace, (const T*)d_cov_trace, (int)n_points, (int)s.point,
                         (const T*)d_grid + s.grid, (const T*)d_grid + s.grid + s.nx, (int)s.nx, (int)s.ny,
                         (const T*)d_misalignment + 2 * k, misalignment_stride, (const T*)d_images_bar + s.cell, list.cells, d_slab);
      HIP_TRY(ctx, hipGetLastError());
      hipLaunchKernelGGL(k_gaussian_image_along_bwd_finish<T>, dim3((unsigned)batch), dim3(64), 0, ctx->stream,
                         (const T*)d_cov_trace, (int)n_points, (int)s.point, (const double*)d_slab, (int)s.chunks, (T*)d_mu_bar,
                         (T*)d_cov_bar, d_grad_misalignment ? (T*)d_grad_misalignment + 2 * k : (T*)nullptr,
                         (int64_t)2 * n_screens);
      HIP_TRY(ctx, hipGetLastError());
    }
    return (int)LYNX_OK;
  });
}

int lynx_gaussian_images_along_mse(lynx_ctx* ctx, int dtype, int64_t batch, int32_t n_points, const void* d_mu_trace,
                                   const void* d_cov_trace, int32_t n_screens, const int32_t* screens, const void* d_grid,
                                   const void* d_misalignment, int64_t misalignment_stride, const int64_t* target_offsets,
                                   const void* d_targets, int64_t target_stride, double* d_loss, double* d_sums) {
  LYNX_MAIN_ENTRY(ctx);
  ImageScreens list;
  if (const int rc = image_screens(ctx, kImageLoss,
                                   d_mu_trace && d_cov_trace && d_grid && d_misalignment && target_offsets && d_targets && d_loss && d_sums,
                                   dtype, batch, n_points, n_screens, screens, misalignment_stride, &list))
    return rc;
  int64_t target_cells = 0, slab = 0;  // the cells the offsets name; the largest slab of one screen (screens reuse it in stream order)
  for (int32_t k = 0; k < n_screens; ++k) {
    const ImageScreen& s = list.rows[k];
    const int64_t offset = target_offsets[k];
    if (offset == -1) continue;
    if (offset < 0)
      return fail(ctx, LYNX_ERR_INVALID, "image loss along the trace: a target's offset is -1 (no target) or not negative");
    target_cells = std::max(target_cells, offset + s.cells);
    slab = std::max(slab, batch * s.chunks * 7);
  }
  if (target_stride != 0 && target_stride < target_cells)
    return fail(ctx, LYNX_ERR_INVALID, "image loss along the trace: the targets' sample stride is 0 or at least the cells the offsets name");
  LYNX_MAIN_WRITES(ctx, kFeedsNoBuild, {{d_loss, (size_t)batch * n_screens * sizeof(double)},
                                        {d_sums, (size_t)batch * n_screens * 6 * sizeof(double)}});
  if (const int rc = ensure_scratch(ctx, ctx->scratch.image_loss, (size_t)slab * sizeof(double))) return rc;
  // (a screen without a target: loss 0 and sums 0)
  HIP_TRY(ctx, hipMemsetAsync(d_loss, 0, (size_t)batch * n_screens * sizeof(double), ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(d_sums, 0, (size_t)batch * n_screens * 6 * sizeof(double), ctx->stream));
  double* d_slab = (double*)ctx->scratch.image_loss.buf;
  for (int32_t k = 0; k < n_screens; ++k) {
    const ImageScreen& s = list.rows[k];
    if (target_offsets[k] < 0) continue;
    with_dtype(dtype, [&](auto zero) {
      using T = decltype(zero);
      hipLaunchKernelGGL(k_gaussian_image_along_mse<T>, dim3((unsigned)s.chunks, (unsigned)batch), dim3(kImageGradThreads), 0,
                         ctx->stream, (const T*)d_mu_trace, (const T*)d_cov_trace, (int)n_points, (int)s.point,
                         (const T*)d_grid + s.grid, (const T*)d_grid + s.grid + s.nx, (int)s.nx, (int)s.ny,
                         (const T*)d_misalignment + 2 * k, misalignment_stride, (const T*)d_targets + target_offsets[k],
                         target_stride, d_slab);
    });
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_gaussian_image_along_mse_finish, dim3((unsigned)batch), dim3(64), 0, ctx->stream,
                       (const double*)d_slab, (int)s.chunks, (int)s.cells, d_loss + k, d_sums + 6 * k, (int)n_screens);
    HIP_TRY(ctx, hipGetLastError());
  }
  return LYNX_OK;
}

int lynx_gaussian_images_along_mse_backward(lynx_ctx* ctx, int dtype, int64_t batch, int32_t n_points, const void* d_cov_trace,
                                            int32_t n_screens, const int32_t* screens, const double* d_sums,
                                            const void* d_loss_bar, void* d_mu_bar, void* d_cov_bar, void* d_grad_misalignment) {
  LYNX_MAIN_ENTRY(ctx);
  ImageScreens list;
  if (const int rc = image_screens(ctx, kImageLossBackward, d_cov_trace && d_sums && d_loss_bar && d_mu_bar && d_cov_bar, dtype, batch,
                                   n_points, n_screens, screens, 0, &list))
    return rc;
  const size_t es = dtype_size(dtype);
  LYNX_MAIN_WRITES(ctx, kFeedsNoBuild, {{d_mu_bar, (size_t)batch * n_points * 7 * es},
                                        {d_cov_bar, (size_t)batch * n_points * 49 * es},
                                        {d_grad_misalignment, (size_t)batch * n_screens * 2 * es}});
  for (int32_t first = 0; first < n_screens; first += kImageLossScreens) {
    const int count = std::min<int32_t>(kImageLossScreens, n_screens - first);
    ImageLossScreens points;
    for (int q = 0; q < kImageLossScreens; ++q) points.point[q] = q < count ? list.rows[first + q].point : 0;
    with_dtype(dtype, [&](auto zero) {
      using T = decltype(zero);
      hipLaunchKernelGGL(k_gaussian_image_along_mse_apply<T>, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, ctx->stream,
                         (const T*)d_cov_trace, batch, (int)n_points, points, (int)first, count, (int)n_screens, d_sums,
                         (const T*)d_loss_bar, (T*)d_mu_bar, (T*)d_cov_bar, (T*)d_grad_misalignment);
    });
    HIP_TRY(ctx, hipGetLastError());
  }
  return LYNX_OK;
}

// ---- the moment loss along a trace ---------------------------------------------------------

// What the two moment loss entries check alike, every refusal in front of anything else -> the number of terms in `*n_terms`.
static int moment_loss_arguments(lynx_ctx* ctx, int dtype, int64_t batch, int32_t n_points, const double* d_records,
                                 const void* d_mu_trace, const void* d_cov_trace, const void* d_energy_trace, int32_t ddof,
                                 int32_t n_target_points, const int32_t* target_points, const double* d_rows, int64_t row_stride,
                                 int* n_terms, int* all_masks) {
  if (!d_energy_trace || !target_points || !d_rows || batch <= 0 || n_points <= 0 || n_target_points <= 0)
    return fail(ctx, LYNX_ERR_INVALID, "moment loss along the trace: bad argument");
  if ((d_records != nullptr) == (d_mu_trace != nullptr || d_cov_trace != nullptr) || (d_mu_trace != nullptr) != (d_cov_trace != nullptr))
    return fail(ctx, LYNX_ERR_INVALID, "moment loss along the trace: the states are records, or mu and cov, not both and not neither");
  if (dtype != LYNX_F32 && dtype != LYNX_F64)
    return fail(ctx, LYNX_ERR_INVALID, "moment loss along the trace: the dtype is float32 or float64");
  if (ddof < 0 || ddof > 1)
    return fail(ctx, LYNX_ERR_INVALID, "moment loss along the trace: ddof is 0 or 1");
  int64_t terms = 0;
  int masks = 0;
  for (int32_t q = 0; q < n_target_points; ++q) {
    const int32_t point = target_points[2 * q], mask = target_points[2 * q + 1];
    if (point < 0 || point >= n_points || (q > 0 && point <= target_points[2 * q - 2]))
      return fail(ctx, LYNX_ERR_INVALID, "moment loss along the trace: the target points lie inside the trace and increase");
    if (mask <= 0 || mask >= (1 << kMomentLossProperties))
      return fail(ctx, LYNX_ERR_INVALID, "moment loss along the trace: a property mask has bits 0 .. 22 and is not 0");
    terms += __builtin_popcount((unsigned)mask);
    masks |= mask;
  }
  if (row_stride != 0 && row_stride != 2 * terms)
    return fail(ctx, LYNX_ERR_INVALID, "moment loss along the trace: the rows' sample stride is 0 or 2 * the number of terms");
  if (batch > 0x7fffffffLL * kMomentLossThreads / kMomentLossPoints)  // (a launch has a thread per sample and point of its chunk)
    return fail(ctx, LYNX_ERR_INVALID, "moment loss along the trace: bad argument (the batch is beyond 2^31 - 1)");
  *n_terms = (int)terms;
  *all_masks = masks;
  return LYNX_OK;
}

// The target points of one launch, by value: points `first` .. `first + count - 1` and the ordinal of each one's first term.
static MomentLossPoints moment_loss_chunk(const int32_t* target_points, int32_t first, int count, int* term) {
  MomentLossPoints chunk;
  for (int q = 0; q < kMomentLossPoints; ++q) {
    chunk.point[q] = q < count ? target_points[2 * (first + q)] : 0;
    chunk.mask[q] = q < count ? target_points[2 * (first + q) + 1] : 0;
    chunk.term[q] = *term;
    *term += __builtin_popcount((unsigned)chunk.mask[q]);
  }
  return chunk;
}

// Between lynx_profile_begin and _end every launch of the two entries is one more entry of lynx_profile_launches, in launch order.
struct ProfiledLaunch {
  lynx_ctx* ctx;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  hipError_t begin() {
    if (!ctx->profiling) return hipSuccess;
    if (const hipError_t e = hipEventCreateWithFlags(&e0, timing_event_flags(ctx))) return e;
    return hipEventCreateWithFlags(&e1, timing_event_flags(ctx));
  }
  void end() {
    if (ctx->profiling) ctx->prof_events.emplace_back(e0, e1);
  }
};

static unsigned moment_loss_blocks(int64_t batch, int count) {
  return (unsigned)((batch * count + kMomentLossThreads - 1) / kMomentLossThreads);
}

int lynx_moments_along_loss(lynx_ctx* ctx, int dtype, int64_t batch, int32_t n_points, const double* d_records,
                            const void* d_mu_trace, const void* d_cov_trace, const void* d_energy_trace, int32_t ddof,
                            int32_t n_target_points, const int32_t* target_points, const double* d_rows, int64_t row_stride,
                            double* d_values, double* d_point_loss, double* d_loss) {
  LYNX_MAIN_ENTRY(ctx);
  if (!d_values || !d_point_loss || !d_loss) return fail(ctx, LYNX_ERR_INVALID, "moment loss along the trace: bad argument");
  int n_terms = 0, masks = 0;
  if (const int rc = moment_loss_arguments(ctx, dtype, batch, n_points, d_records, d_mu_trace, d_cov_trace, d_energy_trace, ddof,
                                           n_target_points, target_points, d_rows, row_stride, &n_terms, &masks))
    return rc;
  LYNX_MAIN_WRITES(ctx, kFeedsNoBuild, {{d_values, (size_t)batch * n_terms * sizeof(double)},
                                        {d_point_loss, (size_t)batch * n_target_points * sizeof(double)},
                                        {d_loss, (size_t)batch * sizeof(double)}});
  int term = 0;
  for (int32_t first = 0; first < n_target_points; first += kMomentLossPoints) {
    const int count = std::min<int32_t>(kMomentLossPoints, n_target_points - first);
    const MomentLossPoints chunk = moment_loss_chunk(target_points, first, count, &term);
    ProfiledLaunch stamp{ctx};
    HIP_TRY(ctx, stamp.begin());
    with_dtype(dtype, [&](auto zero) {
      using T = decltype(zero);
      const auto launch = [&](auto kernel) {
        hipExtLaunchKernelGGL(kernel, dim3(moment_loss_blocks(batch, count)), dim3(kMomentLossThreads), 0u, ctx->stream, stamp.e0,
                              stamp.e1, 0u, d_records, (const T*)d_mu_trace, (const T*)d_cov_trace, (const T*)d_energy_trace, batch,
                              (int)n_points, (int)ddof, chunk, (int)first, count, (int)n_target_points, n_terms, d_rows, row_stride,
                              d_values, d_point_loss);
      };
      if (d_records) launch(k_moment_loss_fwd<T, true>);
      else launch(k_moment_loss_fwd<T, false>);
    });
    HIP_TRY(ctx, hipGetLastError());
    stamp.end();
  }
  ProfiledLaunch stamp{ctx};
  HIP_TRY(ctx, stamp.begin());
  hipExtLaunchKernelGGL(k_moment_loss_finish, dim3((unsigned)((batch + kMomentLossThreads - 1) / kMomentLossThreads)),
                        dim3(kMomentLossThreads), 0u, ctx->stream, stamp.e0, stamp.e1, 0u, (const double*)d_point_loss, batch,
                        (int)n_target_points, d_loss);
  HIP_TRY(ctx, hipGetLastError());
  stamp.end();
  return LYNX_OK;
}

int lynx_moments_along_loss_backward(lynx_ctx* ctx, int dtype, int64_t batch, int32_t n_points, const double* d_records,
                                     const void* d_mu_trace, const void* d_cov_trace, const void* d_energy_trace, int32_t ddof,
                                     int32_t n_target_points, const int32_t* target_points, const double* d_rows,
                                     int64_t row_stride, const double* d_loss_bar, double* d_grad_trace, void* d_mu_bar,
                                     void* d_cov_bar, void* d_energy_bar) {
  LYNX_MAIN_ENTRY(ctx);
  if (!d_loss_bar) return fail(ctx, LYNX_ERR_INVALID, "moment loss along the trace: bad argument");
  int n_terms = 0, masks = 0;
  if (const int rc = moment_loss_arguments(ctx, dtype, batch, n_points, d_records, d_mu_trace, d_cov_trace, d_energy_trace, ddof,
                                           n_target_points, target_points, d_rows, row_stride, &n_terms, &masks))
    return rc;
  if (d_records ? (!d_grad_trace || d_mu_bar || d_cov_bar) : (d_grad_trace || !d_mu_bar || !d_cov_bar))
    return fail(ctx, LYNX_ERR_INVALID, "moment loss along the trace: the cotangents have the form of the states, records or mu and cov");
  if ((masks & kMomentLossEnergy) && !d_energy_bar)
    return fail(ctx, LYNX_ERR_INVALID, "moment loss along the trace: a term that depends on the energy needs the energy's cotangents");
  const size_t es = dtype_size(dtype), points = (size_t)batch * n_points;
  LYNX_MAIN_WRITES(ctx, kFeedsNoBuild, {{d_grad_trace, points * LYNX_MOMENT_STRIDE * sizeof(double)},
                                        {d_mu_bar, points * 7 * es},
                                        {d_cov_bar, points * 49 * es},
                                        {d_energy_bar, points * es}});
  int term = 0;
  for (int32_t first = 0; first < n_target_points; first += kMomentLossPoints) {
    const int count = std::min<int32_t>(kMomentLossPoints, n_target_points - first);
    const MomentLossPoints chunk = moment_loss_chunk(target_points, first, count, &term);
    ProfiledLaunch stamp{ctx};
    HIP_TRY(ctx, stamp.begin());
    with_dtype(dtype, [&](auto zero) {
      using T = decltype(zero);
      const auto launch = [&](auto kernel) {
        hipExtLaunchKernelGGL(kernel, dim3(moment_loss_blocks(batch, count)), dim3(kMomentLossThreads), 0u, ctx->stream, stamp.e0,
                              stamp.e1, 0u, d_records, (const T*)d_mu_trace, (const T*)d_cov_trace, (const T*)d_energy_trace, batch,
                              (int)n_points, (int)ddof, chunk, count, d_rows, row_stride, d_loss_bar, d_grad_trace, (T*)d_mu_bar,
                              (T*)d_cov_bar, (T*)d_energy_bar);
      };
      if (d_records) launch(k_moment_loss_bwd<T, true>);
      else launch(k_moment_loss_bwd<T, false>);
    });
    HIP_TRY(ctx, hipGetLastError());
    stamp.end();
  }
  return LYNX_OK;
}

// ---- synthetic beams -------------------------------------------------------------------

int lynx_fill_gaussian(lynx_ctx* ctx, int dtype, int64_t batch, int64_t n_particles, const double* mu,
                       const double* sigma, uint64_t seed, void* d_p) {
  LYNX_MAIN_ENTRY(ctx);
  if (!d_p || !mu || !sigma || batch <= 0 || n_particles <= 0)
    return fail(ctx, LYNX_ERR_INVALID, "bad argument");
  LYNX_MAIN_WRITES(ctx, kFeedsNoBuild, {{d_p, (size_t)batch * n_particles * 7 * dtype_size(dtype)}});
  GaussArgs g;
  for (int i = 0; i < 6; ++i) {
    g.mu[i] = mu[i];
    g.sigma[i] = sigma[i];
  }
  const int64_t total = batch * n_particles * 7;
  const unsigned grid = (unsigned)std::min<int64_t>((total + 255) / 256, 256 * 32);
  with_dtype(dtype, [&](auto zero) {
    using T = decltype(zero);
    hipLaunchKernelGGL(k_fill_gaussian<T>, dim3(grid), dim3(256), 0, ctx->stream, (T*)d_p, total, seed, g);
  });
  HIP_TRY(ctx, hipGetLastError());
  return LYNX_OK;
}

// wave tiles of 64 lanes x (16 / element size) particles, four to a workgroup
static unsigned wave_tile_grid(int dtype, int64_t total_particles, int max_blocks) {
  const int64_t per_block = 4 * 64 * (16 / (int64_t)dtype_size(dtype));
  return (unsigned)std::min<int64_t>((total_particles + per_block - 1) / per_block, max_blocks);
}

int lynx_fill_gaussian_rows(lynx_ctx* ctx, int dtype, int64_t batch, int64_t n_particles, const double* d_rows,
                            uint64_t seed, void* d_p) {
  LYNX_MAIN_ENTRY(ctx);
  if (!d_p || !d_rows || batch <= 0 || n_particles <= 0 || (dtype != LYNX_F32 && dtype != LYNX_F64) ||
      batch > (int64_t)(0x7fffffffffffffffLL / 14) / n_particles)  // (2 * scalars is the generator's counter)
    return fail(ctx, LYNX_ERR_INVALID, "bad argument");
  LYNX_MAIN_WRITES(ctx, kFeedsNoBuild, {{d_p, (size_t)batch * n_particles * 7 * dtype_size(dtype)}});
  const int64_t total = batch * n_particles;
  const unsigned grid = wave_tile_grid(dtype, total, kBeamFactoryMaxBlocks);
  with_dtype(dtype, [&](auto zero) {
    using T = decltype(zero);
    hipLaunchKernelGGL(k_fill_gaussian_rows<T>, dim3(grid), dim3(256), 0, ctx->stream, (T*)d_p, n_particles, total, d_rows, seed);
  });
  HIP_TRY(ctx, hipGetLastError());
  return LYNX_OK;
}

int lynx_transform_particles(lynx_ctx* ctx, int dtype, int64_t batch, int64_t n_particles, const void* d_p_in,
                             int64_t in_sample_stride, const void* d_rows, void* d_p_out) {
  LYNX_MAIN_ENTRY(ctx);
  if (!d_p_in || !d_rows || !d_p_out || batch <= 0 || n_particles <= 0 || (dtype != LYNX_F32 && dtype != LYNX_F64) ||
      batch > (int64_t)(0x7fffffffffffffffLL / 7 / 8) / n_particles)
    return fail(ctx, LYNX_ERR_INVALID, "bad argument");
  if (in_sample_stride != 0 && in_sample_stride != n_particles * 7)
    return fail(ctx, LYNX_ERR_INVALID, "transform: the incoming sample stride is 0 (one stored sample) or n_particles * 7");
  if (in_sample_stride == 0 && d_p_in == d_p_out)
    return fail(ctx, LYNX_ERR_INVALID, "transform: one stored sample cannot be rescaled in place");
  LYNX_MAIN_WRITES(ctx, kFeedsNoBuild, {{d_p_out, (size_t)batch * n_particles * 7 * dtype_size(dtype)}});
  const int64_t total = batch * n_particles;
  const unsigned grid = wave_tile_grid(dtype, total, kBeamFactoryMaxBlocks);
  with_dtype(dtype, [&](auto zero) {
    using T = decltype(zero);
    hipLaunchKernelGGL(k_transform_particles<T>, dim3(grid), dim3(256), 0, ctx->stream, (const T*)d_p_in, in_sample_stride,
                       (T*)d_p_out, n_particles, total, (const T*)d_rows);
  });
  HIP_TRY(ctx, hipGetLastError());
  return LYNX_OK;
}

// ---- diagnostics: practical HBM ceiling ------------------------------------------------------

int lynx_diag_copy(lynx_ctx* ctx, void* d_dst, const void* d_src, size_t bytes, int repeats, int vec_per_thread,
                   float* avg_ms) {
  LYNX_MAIN_ENTRY(ctx);
  const int per_thread = vec_per_thread >= 100 ? vec_per_thread - 100 : vec_per_thread;  // >= 100: non-temporal stores
  if (!d_dst || !d_src || bytes % 16 || repeats <= 0 || vec_per_thread < 0 || per_thread > 64 ||
      (vec_per_thread >= 100 && per_thread == 0))
    return fail(ctx, LYNX_ERR_INVALID, "bad argument");
  LYNX_MAIN_WRITES(ctx, kFeedsNoBuild, {{d_dst, bytes}});
  const int64_t n_vec = (int64_t)(bytes / 16);
  const int vpt = vec_per_thread;  // 0 = grid-stride
  const unsigned grid = per_thread > 0 ? (unsigned)((n_vec + 256LL * per_thread - 1) / (256LL * per_thread))
                                : (unsigned)std::min<int64_t>((n_vec + 255) / 256, 256 * 16);
  hipLaunchKernelGGL(k_diag_copy, dim3(grid), dim3(256), 0, ctx->stream, (const lynx_f32x4*)d_src,
                     (lynx_f32x4*)d_dst, n_vec, vpt);  // warm-up
  HIP_TRY(ctx, hipEventRecord(ctx->ev_start, ctx->stream));
  for (int r = 0; r < repeats; ++r)
    hipLaunchKernelGGL(k_diag_copy, dim3(grid), dim3(256), 0, ctx->stream, (const lynx_f32x4*)d_src,
                       (lynx_f32x4*)d_dst, n_vec, vpt);
  HIP_TRY(ctx, hipEventRecord(ctx->ev_stop, ctx->stream));
  HIP_TRY(ctx, hipEventSynchronize(ctx->ev_stop));
  float ms = 0.f;
  HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev_start, ctx->ev_stop));
  *avg_ms = ms / repeats;
  return LYNX_OK;
}

// ---- RCCL ------------------------------------------------------------------------------

int lynx_comm_unique_id(char* id_out) {
  static_assert(sizeof(ncclUniqueId) <= LYNX_UNIQUE_ID_BYTES, "unique id does not fit");
  ncclUniqueId id;
  NCCL_TRY(nullptr, ncclGetUniqueId(&id));
  memset(id_out, 0, LYNX_UNIQUE_ID_BYTES);
  memcpy(id_out, &id, sizeof(id));
  return LYNX_OK;
}

int lynx_comm_init(lynx_ctx* ctx, int n_ranks, int rank, const char* id) {
  if (!ctx || !id || n_ranks <= 0 || rank < 0 || rank >= n_ranks) return fail(ctx, LYNX_ERR_INVALID, "bad argument");
  if (ctx->comm) return fail(ctx, LYNX_ERR_INVALID, "communicator already initialised");
  HIP_TRY(ctx, use_device(ctx));
  ncclUniqueId uid;
  memcpy(&uid, id, sizeof(uid));
  NCCL_TRY(ctx, ncclCommInitRank(&ctx->comm, n_ranks, uid, rank));
  ctx->comm_ranks = n_ranks;
  if (n_ranks > 1 && !ctx->plain_events) {  // (a job that did not say WORLD_SIZE: its events get HIP's default fence now)
    HIP_TRY(ctx, hipStreamSynchronize(ctx->s_build));
    HIP_TRY(ctx, sync_main(ctx));
    const int rc = wait_for_side(ctx);
    if (rc) return rc;
    {
      std::lock_guard<std::mutex> lock(ctx->mu);
      retire_side_ops(ctx, true);
    }
    ctx->plain_events = true;
    ctx->last_stream_stop = nullptr;
    return make_sync_events(ctx);
  }
  return LYNX_OK;
}

int lynx_comm_destroy(lynx_ctx* ctx) {
  if (ctx && ctx->comm) {
    HIP_TRY(ctx, sync_main(ctx));
    int rc = wait_for_side(ctx);
    if (rc) return rc;
    NCCL_TRY(ctx, ncclCommDestroy(ctx->comm));
    ctx->comm = nullptr;
    ctx->comm_ranks = 0;
  }
  return LYNX_OK;
}

int lynx_comm_info(lynx_ctx* ctx, int32_t* rccl_version, int32_t* n_ranks, int32_t* rank) {
  if (!ctx || !rccl_version || !n_ranks || !rank) return fail(ctx, LYNX_ERR_INVALID, "null argument");
  int v = 0;
  NCCL_TRY(ctx, ncclGetVersion(&v));
  *rccl_version = v;
  *n_ranks = 0;
  *rank = -1;
  if (ctx->comm) {
    int n = 0, r = -1;
    NCCL_TRY(ctx, ncclCommCount(ctx->comm, &n));
    NCCL_TRY(ctx, ncclCommUserRank(ctx->comm, &r));
    *n_ranks = n;
    *rank = r;
  }
  return LYNX_OK;
}

int lynx_gather_moments(lynx_ctx* ctx, const double* d_send, double* d_recv, int64_t count) {
  LYNX_MAIN_ENTRY(ctx);
  if (!ctx->comm) return fail(ctx, LYNX_ERR_INVALID, "communicator not initialised");
  LYNX_MAIN_WRITES(ctx, kFeedsNoBuild, {{d_recv, (size_t)std::max(1, ctx->comm_ranks) * count * sizeof(double)}});
  // Default with more than one rank: the side stream.  With one rank (LYNX_FORCE_COMM rehearsals) the "gather" is
  // a copy; it follows the reduction wherever that ran.
  const bool produced_on_side = ctx->side_wrote && ctx->side_wrote == (const void*)d_send;
  if (knob(ctx->knobs.gather_overlap, (ctx->comm_ranks > 1 || produced_on_side) ? 1 : 0) == 0) {  // in line, on the main stream
    int rc = join_side(ctx);  // the records may come from a reduction on the side stream
    if (rc) return rc;
    hipEvent_t g0 = nullptr, g1 = nullptr;
    if (ctx->profiling) {
      HIP_TRY(ctx, hipEventCreateWithFlags(&g0, timing_event_flags(ctx)));
      HIP_TRY(ctx, hipEventCreateWithFlags(&g1, timing_event_flags(ctx)));
      HIP_TRY(ctx, hipEventRecord(g0, ctx->stream));
    }
    NCCL_TRY(ctx, ncclAllGather(d_send, d_recv, (size_t)count, ncclDouble, ctx->comm, ctx->stream));
    if (g1) {
      HIP_TRY(ctx, hipEventRecord(g1, ctx->stream));
      ctx->prof_gather_events.emplace_back(g0, g1);
    }
    return LYNX_OK;
  }
  // The gather is latency (a few hundred KB over xGMI, and it couples this GPU to the slowest rank of the step) and
  // nothing on this GPU waits for its result but the host: it runs on the side stream, underneath the next call's
  // streaming kernel, instead of between two of them.  In line every rank would run in lockstep with the slowest
  // one, step by step; decoupled only the end of the job waits for everybody.
  //   start : when the records are final -- stream order when the side stream reduced them itself, else a marker
  //           behind everything enqueued on the main stream so far;
  //   end   : a "done" event; the main stream never waits for it.  The two blocks stay out of the allocator until it
  //           has fired (ctx_free defers them), the host sees the result through lynx_buf_d2h / lynx_sync, which
  //           wait for this stream.
  if (!produced_on_side) {
    HIP_TRY(ctx, hipEventRecord(ctx->ev_main_mark, ctx->stream));
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->s_side, ctx->ev_main_mark, 0));
  }
  hipEvent_t done = nullptr;
  int rc = side_event(ctx, &done);
  if (rc) return rc;
  hipEvent_t g0 = nullptr, g1 = nullptr;
  if (ctx->profiling) {  // the gather's own duration on its stream (bench.py at N > 1: how long a rank waits for the others)
    HIP_TRY(ctx, hipEventCreateWithFlags(&g0, timing_event_flags(ctx)));
    HIP_TRY(ctx, hipEventCreateWithFlags(&g1, timing_event_flags(ctx)));
    HIP_TRY(ctx, hipEventRecord(g0, ctx->s_side));
  }
  NCCL_TRY(ctx, ncclAllGather(d_send, d_recv, (size_t)count, ncclDouble, ctx->comm, ctx->s_side));
  if (g1) {
    HIP_TRY(ctx, hipEventRecord(g1, ctx->s_side));
    ctx->prof_gather_events.emplace_back(g0, g1);
  }
  HIP_TRY(ctx, hipEventRecord(done, ctx->s_side));
  side_op_issued(ctx, done, d_send, d_recv);
  return LYNX_OK;
}


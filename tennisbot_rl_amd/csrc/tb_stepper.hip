// tb_stepper.hip -- the host side of libtb_stepper.so: the handle, the launches (which kernel instantiation runs when, on which
// stream, behind which event) and the C ABI of include/tb_stepper.h. The kernels themselves are in tb_kernels.hpp (env logic,
// __global__ entry points), tb_device.hpp (one substep of the rigid-body model) and tb_policy.hpp (MlpPolicy towers on MFMA).
//
// Data layout in HBM (DESIGN.md "Layout"): persistent state is structure-of-arrays along
// the env index, 32-bit words [W][N] (W = 30 Swing / 28 Tennisbot) plus one done byte [N],
// so lane i of a wave reads word k at base + (k*N + i)*4: every row access is one fully
// coalesced 256-B wave transaction. Per-call I/O keeps the caller's natural row-major
// shapes (actions [N][A], obs [N][O]); a lane's 8/24/48-byte row is read/written with
// 8- or 16-byte vector accesses and the rows of a wave are contiguous.
//
// Kernel shape: one lane = one world, state held in registers for the whole call
// (including the <= 775-substep SwingRacket fast-forward, swingracket_env.py:105-141, and
// the T steps of tb_rollout). No inter-lane communication except wave-level counter
// reductions; no inter-workgroup communication at all, so blockIdx -> XCD placement does
// not matter for correctness or reuse (there is no shared tile to keep in one L2).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <chrono>
#include <type_traits>

#include "../../include/tb_stepper.h"
#include "tb_device.hpp"

#include "tb_kernels.hpp"
#include "tb_es.hpp"
#include "tb_learner.hpp"
#include "tb_trpo.hpp"
#include "tb_sac.hpp"
#include "tb_tqc.hpp"
#include "tb_render.hpp"
#include "tb_trace.hpp"

using namespace tb;

namespace {

// ------------------------------------------------------------------------------------------
// host side
thread_local char g_err[512] = "";

int fail(int code, const char* what) {
  if (code > 0) snprintf(g_err, sizeof g_err, "%s: %s (%s)", what, hipGetErrorString((hipError_t)code), hipGetErrorName((hipError_t)code));
  else snprintf(g_err, sizeof g_err, "%s", what);
  return code;
}
#define HIP_TRY(expr)                                              \
  do {                                                             \
    hipError_t _e = (expr);                                        \
    if (_e != hipSuccess) return fail((int)_e, #expr);             \
  } while (0)

struct DeviceGuard {  // calls run on the handle's device without disturbing the caller's current device
  int prev = -1;
  bool switched = false;
  hipError_t err = hipSuccess;
  DeviceGuard() = default;  // (no device yet: learner_device enters it once the index is known to exist)
  explicit DeviceGuard(int dev) { enter(dev); }
  void enter(int dev) {
    err = hipGetDevice(&prev);
    if (err == hipSuccess && prev != dev) { err = hipSetDevice(dev); switched = err == hipSuccess; }
  }
  ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
};

bool kind_ok(int k) { return k == TB_ENV_SWING || k == TB_ENV_TENNIS; }

int validate_params(const TbParams* p) {
  if (p->n_hull < 3 || p->n_hull > TB_MAX_HULL) return fail(TB_E_PARAMS, "TbParams.n_hull must be in [3, 64]");
  if (!(p->dt > 0.0f) || !(p->inv_dt > 0.0f)) return fail(TB_E_PARAMS, "TbParams.dt / inv_dt must be positive");
  if (!(p->racket_inv_mass > 0.0f) || !(p->ball_inv_mass > 0.0f) || !(p->ball_inv_inertia > 0.0f)) return fail(TB_E_PARAMS, "TbParams masses must be positive");
  for (int i = 0; i < 3; ++i)
    if (!(p->racket_inertia[i] > 0.0f) || !(p->racket_inv_inertia[i] > 0.0f)) return fail(TB_E_PARAMS, "TbParams.racket_inertia must be positive");
  if (!(p->ball_radius > 0.0f) || !(p->contact_threshold >= 0.0f)) return fail(TB_E_PARAMS, "TbParams.ball_radius / contact_threshold invalid");
  if (p->solver_iters < 1 || p->solver_iters > 1000) return fail(TB_E_PARAMS, "TbParams.solver_iters must be in [1, 1000]");
  if (!(p->solver_tol >= 0.0f)) return fail(TB_E_PARAMS, "TbParams.solver_tol must be >= 0");
  return TB_OK;
}

void to_kparams(const TbParams* p, KParams* k, float* planes) {
  k->dt = p->dt; k->inv_dt = p->inv_dt; k->gravity = p->gravity; k->lin_damp = p->lin_damp; k->ang_damp = p->ang_damp; k->lin_damp_quad = p->lin_damp_quad; k->ang_damp_quad = p->ang_damp_quad;
  k->max_ang_step = p->max_ang_step; k->rest_vel_threshold = p->rest_vel_threshold; k->erp = p->erp;
  k->contact_threshold = p->contact_threshold; k->solver_iters = p->solver_iters; k->flags = p->flags; k->solver_tol = p->solver_tol;
  k->racket_inv_mass = p->racket_inv_mass;
  for (int i = 0; i < 3; ++i) {
    k->racket_inertia[i] = p->racket_inertia[i]; k->racket_inv_inertia[i] = p->racket_inv_inertia[i];
    k->racket_com[i] = p->racket_com[i]; k->ground_half[i] = p->ground_half[i]; k->net_half[i] = p->net_half[i];
  }
  k->racket_half_thick = p->racket_half_thick; k->hull_margin = p->hull_margin; k->hull_bound_radius = p->hull_bound_radius; k->racket_scale = p->racket_scale;
  k->ball_inv_mass = p->ball_inv_mass; k->ball_inv_inertia = p->ball_inv_inertia; k->ball_radius = p->ball_radius;
  k->magnus_k = p->magnus_k; k->ball_spin_max = p->ball_spin_max;
  k->rest_racket = p->rest_racket; k->rest_court = p->rest_court; k->rest_goal = p->rest_goal;
  k->fric_racket = p->fric_racket; k->fric_court = p->fric_court; k->fric_goal = p->fric_goal;
  k->rest_racket_court = p->rest_racket_court; k->fric_racket_court = p->fric_racket_court; k->racket_ground_threshold = p->racket_ground_threshold;
  k->roll_racket = p->roll_racket; k->roll_court = p->roll_court; k->roll_goal = p->roll_goal;
  k->goal_radius = p->goal_radius; k->goal_half_len = p->goal_half_len;
  k->n_hull = p->n_hull;
  float top = p->ground_half[2] > p->goal_half_len ? p->ground_half[2] : p->goal_half_len;
  if ((p->flags & TB_F_NET) && p->net_half[2] > top) top = p->net_half[2];
  k->static_top = top;
  {  // cull planes: 8 fixed directions + the 4 longest edges, each pushed out by its own rounding
    int np = 0;
    auto put_plane = [&](double ny, double nz) {  // (ny, nz, the outline's support value along it)
      double hmax = -1e30;
      for (int i = 0; i < p->n_hull; ++i) { double v = ny * p->hull_edges[i][0] + nz * p->hull_edges[i][1]; hmax = v > hmax ? v : hmax; }
      planes[3 * np] = (float)ny; planes[3 * np + 1] = (float)nz; planes[3 * np + 2] = (float)(hmax + 1e-6); ++np;
    };
    for (int d = 0; d < 8; ++d) { const double ang = d * 0.78539816339744830962; put_plane(cos(ang), sin(ang)); }
    bool used[TB_MAX_HULL] = {false};
    for (int pick = 0; pick < TB_N_CULL - 8; ++pick) {
      int best = -1; double bl = -1.0;
      for (int i = 0; i < p->n_hull; ++i) {
        double l2 = (double)p->hull_edges[i][2] * p->hull_edges[i][2] + (double)p->hull_edges[i][3] * p->hull_edges[i][3];
        if (!used[i] && l2 > bl) { bl = l2; best = i; }
      }
      used[best] = true;
      const double il = 1.0 / sqrt(bl);
      put_plane(p->hull_edges[best][3] * il, -p->hull_edges[best][2] * il);  // outward normal of a CCW edge
    }
  }
  // same float operations as the rows would do per contact (oracle setup_row): bit-identical
  k->ball_kn = 1.0f / p->ball_inv_mass;
  k->ball_kt = 1.0f / fmaf(p->ball_inv_inertia, p->ball_radius * p->ball_radius, p->ball_inv_mass);
}

// test hook (tb_diag_fail_alloc): the n-th device allocation of the pipeline or the pool (tb_set_pipeline, tb_set_params) fails with hipErrorOutOfMemory
int g_fail_alloc_countdown = 0;
hipError_t pipeline_malloc(void** p, size_t bytes) {
  if (g_fail_alloc_countdown > 0 && --g_fail_alloc_countdown == 0) { *p = nullptr; return hipErrorOutOfMemory; }
  return hipMalloc(p, bytes);
}
hipError_t pipeline_calloc(void** p, size_t bytes) { const hipError_t e = pipeline_malloc(p, bytes); return e == hipSuccess ? hipMemset(*p, 0, bytes) : e; }  // ... zeroed

// a kernel launch and its check (the stepping launches clear a stale sticky error first: their check is about THIS launch)
template <class... P, class... A>
int launch(void (*kern)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t q, const A&... args) {
  hipLaunchKernelGGL(kern, grid, block, lds, q, args...);
  HIP_TRY(hipGetLastError());
  return TB_OK;
}
// free / destroy what is there, and forget it
template <class T> void drop(T*& p) { if (p) (void)hipFree(p); p = nullptr; }
void drop(hipEvent_t& e) { if (e) (void)hipEventDestroy(e); e = nullptr; }
void drop(hipStream_t& q) { if (q) (void)hipStreamDestroy(q); q = nullptr; }
// None: work issued to `s` runs; Active: it only becomes a node of the graph being captured
int capture_status(hipStream_t s, hipStreamCaptureStatus* st) { *st = hipStreamCaptureStatusNone; HIP_TRY(hipStreamIsCapturing(s, st)); return TB_OK; }

#define TB_FF_SLOTS 8  // parked-state buffers + side streams: ~2.5 fast-forwards are in flight in steady state
#define TB_PIPELINE_MAX_ENVS (1 << 24)
#define TB_DEFER_MAX_ENVS 131072  // deferred stragglers: a small-batch scheme (large batches run the fast-forward in phases)
#define TB_TWO_WAVE_MAX_ENVS 16384  // the two-wave step kernel up to here (auto)
constexpr int kEpisodeSteps = 26;  // a SwingRacket episode is exactly this many agent steps (the kernels keep their own 25 / 26)
static_assert(kEpisodeSteps == episode_cap(TB_ENV_SWING), "the whole-episode kernels' trip limit is the episode's length");
constexpr size_t kSealedWord = (size_t)TB_N_COUNTERS * TB_COUNTER_SHARDS;  // the counter block: [TB_COUNTER_SHARDS][TB_N_COUNTERS] ...
constexpr size_t kCounterWords = kSealedWord + 1;  // ... + one word: substeps booked by the pool's sealed-fate exit

// The scheduler's parts: plain data, all zero = never built (the handle is calloc'ed).
// Episode phase: agent steps since the last full reset, known while every env is in lockstep
struct Phase {
  int at, valid, at_capture, valid_at_capture;  // ..._at_capture: snapshot taken by tb_pipeline_sync(h, 1), restored by tb_pipeline_sync(h, 0) / tb_pipeline_recover
  void set(int steps) { valid = 1; at = steps; }
  void invalidate() { valid = 0; }
  void advance(int T) { if (valid) at = (at + T) % kEpisodeSteps; }
  bool launch_ends_episode(int T) const { return at + T == kEpisodeSteps; }
  int chunk(int left) const { const int room = kEpisodeSteps - at; return left < room ? left : room; }  // a launch ends where the episodes end
  void save_for_capture() { at_capture = at; valid_at_capture = valid; }
  void restore() { at = at_capture; valid = valid_at_capture; }
};

// One fast-forward slot: a side stream, the events that fork it from the caller's stream and close its work, the parking buffers
struct FfSlot {
  hipStream_t side;  // one stream per slot: consecutive fast-forwards overlap each other too
  hipEvent_t ev_step, ev_ff;
  int busy;
  float4* rec;       // [n][ff_rec<RG>()] parked records (park_env), allocated for TB_FF_REC_MAX
  uint8_t* flag;     // [n] parked flags
  float4* list[2];   // survivors of fast-forward phases 1 and 2 (worst case: every env), compacted
  int* count;        // [2] their numbers
  // fast-forwards enqueued on this slot (= per side stream: only there is "the first k have finished" the same as "k have
  // finished" -- fast-forwards of different episodes overtake each other, one with a ball at rest on a grounded racket
  // runs five times as long as the next): inside the current / latest capture; eagerly since tb_mark_begin
  long long in_capture, eager;
  int open() {
    HIP_TRY(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&ev_step, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&ev_ff, hipEventDisableTiming));
    return TB_OK;
  }
  void close() { drop(side); drop(ev_step); drop(ev_ff); busy = 0; }
  int build(int n, int phases) {
    if (int rc = open()) return rc;
    const size_t wb = sizeof(float4) * (size_t)TB_FF_REC_MAX * n;
    HIP_TRY(pipeline_calloc((void**)&rec, wb));
    HIP_TRY(pipeline_calloc((void**)&flag, (size_t)n));
    for (int ph = 0; ph + 1 < phases; ++ph) HIP_TRY(pipeline_malloc((void**)&list[ph], wb));
    HIP_TRY(pipeline_calloc((void**)&count, 2 * sizeof(int)));
    return TB_OK;
  }
  void free_buffers() { drop(rec); drop(flag); drop(list[0]); drop(list[1]); drop(count); }
};

struct Slots {
  FfSlot s[TB_FF_SLOTS];
  int next, last;                    // the slot the next parking launch takes; the one that closed last (-1: none to order against)
  const void *last_term, *last_sub;  // shared late-written buffers force ordering between fast-forwards
  bool built() const { return s[0].side != nullptr; }
  int claim() { const int k = next; next = (k + 1) % TB_FF_SLOTS; return k; }
  // what was enqueued before no longer orders what comes next (joined by the host, or on the other side of a capture boundary)
  void forget_ordering() { for (FfSlot& f : s) f.busy = 0; last = -1; last_term = nullptr; last_sub = nullptr; }
  void forget_capture() { for (FfSlot& f : s) f.in_capture = 0; }
};

// Deferred stragglers (tb_ff_kernel<.., POOL>; TbOptions.ff_defer): one pool for all episodes between two flushes.
// 64 n records (two reference-sized rollouts of 1100 steps with EVERY episode end in it) + the slack
// all resident fast-forward waves could overshoot it by (slots x n), 192 B each + an 8-byte destination pointer: 14 KB per env.
// Allocated only for handles whose defer_mode can be non-zero: on request, up to 16384 envs, or above that (to 131072) once the
// parameter block turns racket<->court contact on -- tb_set_params asks again, with the new flags, before it commits them. (Until round 4 every pipelined handle up
// to 131072 envs got one: 1.9 GB at that size that the default kernels never touched.) Zeroed: a record's tag word says whether
// it holds a parked env, and no launch may ever find a tag it did not write.
struct Pool {
  float4* rec;             // [cap + slack][TB_FF_REC_MAX]; non-null = a usable pool (all of it or none)
  float** dst;             // [cap + slack] where each deferred env's terminal reward goes
  int* count;
  int cap, slack, pending;  // pending: records may be waiting (the next flush runs the pool kernel)
  int run_upto;            // ... of which the first run_upto have had their launch already (at a progress mark)
  int episodes;            // ff_defer = 2: episodes parked straight into the pool since the last flush (records [k n, (k + 1) n) each)
  hipEvent_t ev_direct;    // ... and the latest launch that did so (a flush on another stream waits for it)
  hipEvent_t ev_run;       // the last pool run (+ the reset of its counter): later fast-forwards append behind it, whatever stream flushed
  int run_ev_valid, direct_ev_valid;
  size_t records() const { return (size_t)cap + (size_t)slack; }
  void idle() { pending = 0; episodes = 0; run_upto = 0; }             // nothing is waiting for a pool run
  void events_forgotten() { run_ev_valid = 0; direct_ev_valid = 0; }  // (an event recorded on one side of a capture boundary means nothing on the other)
  int build(int n) {  // into a zeroed local value: the caller swaps it in on success and releases it otherwise
    cap = 64 * n; slack = TB_FF_SLOTS * n;
    HIP_TRY(pipeline_calloc((void**)&rec, sizeof(float4) * (size_t)TB_FF_REC_MAX * records()));
    HIP_TRY(pipeline_calloc((void**)&dst, sizeof(float*) * records()));
    HIP_TRY(pipeline_calloc((void**)&count, sizeof(int)));
    HIP_TRY(hipEventCreateWithFlags(&ev_run, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&ev_direct, hipEventDisableTiming));
    return TB_OK;
  }
  void release() { drop(rec); drop(dst); drop(count); drop(ev_run); drop(ev_direct); *this = Pool{}; }
};

// Progress marks (tb_mark_record). h: pinned host counters written by tb_mark_kernel -- [k] firings of mark k
// (a kernel on the caller's own stream), [TB_MAX_MARKS + slot] fast-forwards finished (a kernel behind every tb_ff_kernel on
// its side stream). No extra streams, no extra graph edges: a mark never makes anything wait. What a mark still has
// to wait for -- the fast-forwards enqueued before it -- is host arithmetic over these two kinds of counters.
struct Marks {
  unsigned long long* h;
  unsigned long long snap_ff[TB_FF_SLOTS], snap_marks[TB_MAX_MARKS];  // the counters at tb_mark_begin (nothing of this handle in flight)
  int on;                                       // tb_mark_enable: fast-forwards are followed by their counting kernel
  long long ff_before[TB_MAX_MARKS][TB_FF_SLOTS];  // fast-forwards enqueued per slot before the mark: inside a capture FfSlot::in_capture at that point, eagerly FfSlot::eager (in_capture says which)
  int in_capture[TB_MAX_MARKS];
  int ensure() {
    if (h) return TB_OK;
    HIP_TRY(hipHostMalloc((void**)&h, sizeof(unsigned long long) * (TB_MAX_MARKS + TB_FF_SLOTS), hipHostMallocDefault));
    memset(h, 0, sizeof(unsigned long long) * (TB_MAX_MARKS + TB_FF_SLOTS));
    return TB_OK;
  }
};

}  // namespace

struct TbHandle {
  int device, kind, n, block;
  TbOptions opt;  // as given to tb_create (0 = auto)
  int two_wave;  // the pipelined SwingRacket one-step kernel in its two-wave form (tb_kernels.hpp, two_wave_step)
  uint64_t seed, env_id_base;
  TbParams params;
  KParams kp;
  uint32_t* d_words;
  uint8_t* d_done;
  float4* d_hull;
  float4* h_hull;  // pinned staging copy of the outline table
  float cull_planes[TB_N_CULL][3];  // derived from the outline (to_kparams); they travel behind it in the same table
  unsigned long long* d_counters;     // [kCounterWords]
  uint32_t* d_mani;                   // [TB_MANI_WORDS][n] racket<->court contact caches
  uint8_t* d_mflag;                   // [n]
  int params_generation;   // tb_set_params count: captured launches carry the parameter block they were captured with
  unsigned long long first_substeps;  // counters[6], the host's share: n envs x agent steps of every launch that RAN (see count_first_substeps)
  float* d_es_rew;  // [n] tb_es_evaluate: where the fast-forward writes the 26th step's reward (allocated on first use)
  // pipelined fast-forward
  int pipeline;                   // enabled by tb_set_pipeline
  int ff_phases;                  // 1 = one kernel runs every loop to its end; 2, 3 = budgeted phases + survivor kernels
  int ff_lanes;                   // parked envs per wave of tb_ff_kernel's first phase (TbOptions.ff_lanes_per_wave, or chosen from n)
  Phase phase;
  Slots slots;
  Pool pool;
  Marks marks;
};

namespace {

int words_of(int kind) { return kind == TB_ENV_SWING ? TB_SWING_WORDS : TB_TENNIS_WORDS; }

// dynamic LDS of a stepping kernel: `words` per lane (the kernel family's *_lds_words, tb_kernels.hpp) for `lanes` lanes
#ifdef TB_DIAG_LDS_PAD  // (tools/diag/r03_occupancy_probe.py: fewer workgroups per CU through a padded dynamic LDS request; tb_diag_set_lds_pad)
size_t g_diag_lds_pad = 0;
#else
constexpr size_t g_diag_lds_pad = 0;
#endif
size_t dyn_lds(int words, unsigned lanes) { return g_diag_lds_pad + sizeof(float) * lanes * words; }

// 128-thread workgroups, measured with 64 / 128 / 256 alternated in one process (tools/diag/diag_blocks2.py; M env steps/s):
//   SwingRacket  4096: 662-679 / 673-684 / 657-682    32768: 4570 / 4760 / 3600    65536: 4900 / 4600 / 4250    131072: 5900 / 5760 / 5450
//                262144: 7630 / 7630 / 7390            1 M: 8980 / 9000 / 8830
//   Tennisbot    4096: 667 / 666 / 669    32768: 3736 / 3825 / 3800    65536: 6300 / 6350 / 6430    262144: 13250 / 13450 / 13390    1 M: 18400 / 18900 / 18300
// i.e. 128 everywhere but for SwingRacket between 64 K and 128 K envs, where one wave per workgroup wins by 2-6 %.
int pick_block(int kind, int n, const TbOptions& o) {
  if (o.block == 64 || o.block == 128 || o.block == 256) return o.block;
  // (round 3, final build, no barrier left in the one-substep kernels: one-wave workgroups win up to 16384 envs -- SwingRacket 4096 envs
  //  1052 against 1033 M env steps/s, 16384: 3.07 / 3.01 G, Tennisbot 4096: 738 / 733 M, 8192: 1.24 / 1.23 G; 32768: 5.65 / 5.68 and 3.78 / 3.82 G)
  if (n <= 16384) return 64;
  return kind == TB_ENV_SWING && n >= 49152 && n <= 131072 ? 64 : 128;
}

// the parameter side of the pool's sealed-fate exit (fate_sealed in tb_kernels.hpp states the argument these limits belong to)
bool seal_params_ok(const TbHandle* h) {
  const KParams& k = h->kp;
  if (h->opt.ff_seal < 0 || h->kind != TB_ENV_SWING || !(k.flags & TB_F_AUTO_RESET) || k.magnus_k != 0.0f) return false;
  if (!(k.dt > 0.0f) || !(k.gravity > 0.0f) || !(k.racket_inv_mass > 0.0f) || !(k.lin_damp >= 0.0f) || !(k.lin_damp_quad >= 0.0f)) return false;
  const double wdt2 = 50.0 * (double)k.racket_inv_mass * (double)k.dt * (double)k.dt;      // (w dt)^2 of the stiffer axis
  const double c_max = (double)k.dt * ((double)k.lin_damp + 1000.0 * (double)k.lin_damp_quad);  // drag per substep at the 1000 m/s the test admits
  return wdt2 <= 0.04 && c_max <= 0.2;
}

KArgs base_args(const TbHandle* h) {
  KArgs a;
  memset(&a, 0, sizeof a);
  a.P = h->kp; a.words = h->d_words; a.done_state = h->d_done; a.hull = h->d_hull; a.counters = h->d_counters;
  a.ff_sealed = seal_params_ok(h) ? h->d_counters + kSealedWord : nullptr;
  a.mani = h->d_mani; a.mflag = h->d_mflag;
  a.seed = h->seed; a.env_id_base = h->env_id_base; a.n = h->n; a.T = 1;
  return a;
}

int upload_hull(TbHandle* h, hipStream_t s) {
  memcpy(h->h_hull, h->params.hull_edges, sizeof(float) * TB_HULL_REC * TB_MAX_HULL);
  memcpy(reinterpret_cast<float*>(h->h_hull + TB_HULL_PLANES), h->cull_planes, sizeof h->cull_planes);
  memset(h->h_hull + TB_HULL_KP, 0, sizeof(float4) * TB_KP_ROWS);
  memcpy(h->h_hull + TB_HULL_KP, &h->kp, sizeof h->kp);
  HIP_TRY(hipMemcpyAsync(h->d_hull, h->h_hull, sizeof(float4) * TB_HULL_LDS, hipMemcpyHostToDevice, s));
  return TB_OK;
}

// make `s` wait for every fast-forward still running on the side stream
int wait_side(TbHandle* h, hipStream_t s) {
  for (const FfSlot& f : h->slots.s)
    if (f.busy) HIP_TRY(hipStreamWaitEvent(s, f.ev_ff, 0));
  return TB_OK;
}

// the RG template instantiations hold what the default kernels leave out: racket <-> court contact and rolling friction
bool extended_contacts(const KParams& kp) {
  return (kp.flags & TB_F_RACKET_GROUND) || kp.roll_racket > 0.0f || kp.roll_court > 0.0f || kp.roll_goal > 0.0f;
}

// a pool record's size in float4s under the handle's contact set: the host side of ff_rec<RG>() (allocated for TB_FF_REC_MAX)
size_t pool_rec(const TbHandle* h) { return extended_contacts(h->kp) ? ff_rec<true>() : ff_rec<false>(); }

// Kernel selectors: the instantiation that runs a launch's variant. They reach exactly the variants the launches below ask for;
// any other is null (nothing is built for it) and its launch fails.
using StepKernel = void (*)(const uint32_t*, const uint8_t*, const float*, const float4*, int, int, KArgs);
using ArgsKernel = void (*)(KArgs);

// tb_step_kernel<KIND, LEAN, MULTI, RG, POLICY>; the fused policy step runs one step per launch (Tennisbot: with either network)
template <int KIND, bool LEAN>
StepKernel step_kernel_of(bool multi, bool rg, bool pol, int net) {
  if constexpr (KIND == TB_ENV_TENNIS) {
    if (pol && net == TB_NET_TUNED)
      return multi ? nullptr : rg ? tb_step_kernel<KIND, LEAN, false, true, true, false, TB_NET_TUNED> : tb_step_kernel<KIND, LEAN, false, false, true, false, TB_NET_TUNED>;
  }
  if constexpr (KIND == TB_ENV_SWING) {
    if (pol && net == TB_NET_MLP64)
      return multi ? nullptr : rg ? tb_step_kernel<KIND, LEAN, false, true, true, false, TB_NET_MLP64> : tb_step_kernel<KIND, LEAN, false, false, true, false, TB_NET_MLP64>;
  }
  if (net != TB_NET_DEFAULT) return nullptr;
  if (pol) return multi ? nullptr : rg ? tb_step_kernel<KIND, LEAN, false, true, true> : tb_step_kernel<KIND, LEAN, false, false, true>;
  if (multi) return rg ? tb_step_kernel<KIND, LEAN, true, true> : tb_step_kernel<KIND, LEAN, true, false>;
  return rg ? tb_step_kernel<KIND, LEAN, false, true> : tb_step_kernel<KIND, LEAN, false, false>;
}
// ... and <.., TWO_WAVE> where the variant has that form (step_has_two_waves); LEAN is SwingRacket's only
StepKernel step_kernel(int kind, bool lean, bool multi, bool rg, bool pol, bool two_wave, int net) {
  if (two_wave) return step_has_two_waves(kind, lean, multi, rg, pol) ? tb_step_kernel<TB_ENV_SWING, true, false, false, false, true> : nullptr;
  if (kind == TB_ENV_TENNIS) return lean ? nullptr : step_kernel_of<TB_ENV_TENNIS, false>(multi, rg, pol, net);
  return lean ? step_kernel_of<TB_ENV_SWING, true>(multi, rg, pol, net) : step_kernel_of<TB_ENV_SWING, false>(multi, rg, pol, net);
}

// tb_ff_kernel<RG, BIG, ESC, POOL>: ESC only as the first of a BIG fast-forward's phases; a BIG POOL only without RG
ArgsKernel ff_kernel(bool rg, bool big, bool esc, bool pool) {
  if (esc) return !big || pool ? nullptr : rg ? tb_ff_kernel<true, true, true> : tb_ff_kernel<false, true, true>;
  if (pool) return rg ? (big ? nullptr : tb_ff_kernel<true, false, false, true>) : big ? tb_ff_kernel<false, true, false, true> : tb_ff_kernel<false, false, false, true>;
  if (rg) return big ? tb_ff_kernel<true, true> : tb_ff_kernel<true, false>;
  return big ? tb_ff_kernel<false, true> : tb_ff_kernel<false, false>;
}

// The loop kernels' selectors. `pick` is a generic lambda that names the kernel template once, with its parameters taken from the
// types of its arguments: [](auto K, auto R) { return tb_es_rollout_kernel<K.value, R.value>; }
template <int V> using Int = std::integral_constant<int, V>;
// (kind, RG): tb_es_rollout_kernel, tb_sac_evaluate_kernel, tb_sac_collect_kernel
template <class F>
auto kernel_of_kind_rg(int kind, bool rg, F pick) {
  if (kind == TB_ENV_SWING) return rg ? pick(Int<TB_ENV_SWING>{}, std::true_type{}) : pick(Int<TB_ENV_SWING>{}, std::false_type{});
  return rg ? pick(Int<TB_ENV_TENNIS>{}, std::true_type{}) : pick(Int<TB_ENV_TENNIS>{}, std::false_type{});
}
// THE (kind, net) PAIRS THE POLICY AND LEARNER KERNELS ARE BUILT FOR: every kind's own network, SwingRacket's [64, 64], Tennisbot's tuned
// one. f(Int<KIND>{}, Int<NET>{}) for those -- a layout's constant, a kernel, a launch --, `otherwise` for any other pair. policy_net_ok
// asks this table too, so what it lets through has an entry.
template <class T, class F>
T with_kind_net(int kind, int net, T otherwise, F f) {
  if (kind == TB_ENV_SWING && net == TB_NET_DEFAULT) return f(Int<TB_ENV_SWING>{}, Int<TB_NET_DEFAULT>{});
  if (kind == TB_ENV_SWING && net == TB_NET_MLP64) return f(Int<TB_ENV_SWING>{}, Int<TB_NET_MLP64>{});
  if (kind == TB_ENV_TENNIS && net == TB_NET_DEFAULT) return f(Int<TB_ENV_TENNIS>{}, Int<TB_NET_DEFAULT>{});
  if (kind == TB_ENV_TENNIS && net == TB_NET_TUNED) return f(Int<TB_ENV_TENNIS>{}, Int<TB_NET_TUNED>{});
  return otherwise;
}
// (kind, net, RG): tb_policy_evaluate_kernel, tb_policy_rollout_kernel; null for a pair without an entry, and its launch a refusal
template <class F>
auto kernel_of_kind_net_rg(int kind, int net, bool rg, F pick) {
  using Kernel = decltype(pick(Int<TB_ENV_SWING>{}, Int<TB_NET_DEFAULT>{}, std::false_type{}));
  return with_kind_net(kind, net, Kernel(nullptr), [&](auto K, auto N) -> Kernel { return rg ? pick(K, N, std::true_type{}) : pick(K, N, std::false_type{}); });
}

// the fast-forward family's one launch: one-wave workgroups on stream q
int launch_ff_kernel(bool rg, bool big, bool esc, bool pool, dim3 grid, size_t lds, hipStream_t q, const KArgs& k) {
  const ArgsKernel kern = ff_kernel(rg, big, esc, pool);
  if (!kern) return fail(TB_E_UNSUPPORTED, "no tb_ff_kernel instantiation for this variant");
  return launch(kern, grid, dim3(64), lds, q, k);
}

// Work on the side stream of `slot` forks from `s` (it runs after everything issued to `s` so far) ...
int fork_side(FfSlot& f, hipStream_t s) {
  HIP_TRY(hipEventRecord(f.ev_step, s));
  HIP_TRY(hipStreamWaitEvent(f.side, f.ev_step, 0));
  return TB_OK;
}
// ... and closes with its progress-mark count, the slot's event and the bookkeeping that later launches order themselves by;
// `term` / `substeps`: the late-written buffers that the work writes (or null)
int close_side(TbHandle* h, int slot, const void* term, const void* substeps, hipStream_t s) {
  FfSlot& f = h->slots.s[slot];
  if (h->marks.h && h->marks.on) {  // progress marks: count this fast-forward as finished, in stream order behind it
    if (int rc = launch(tb_mark_kernel, dim3(1), dim3(1), 0, f.side, h->marks.h + TB_MAX_MARKS + slot)) return rc;
    hipStreamCaptureStatus st;
    if (int rc = capture_status(s, &st)) return rc;
    if (st == hipStreamCaptureStatusActive) f.in_capture++; else f.eager++;
  }
  HIP_TRY(hipEventRecord(f.ev_ff, f.side));
  f.busy = 1; h->slots.last = slot; h->slots.last_term = term; h->slots.last_sub = substeps;
  return TB_OK;
}

// finish the lanes parked in `slot` on that slot's side stream, ordered after everything issued to `s` so far
// (Measured and dropped in round 3: enqueueing the fast-forward one launch LATE, so that under stream capture the next step -- not
//  the fast-forward -- is the parking node's first successor. It does what was hoped for the chain -- all 2132 step kernels of two
//  replays on ONE hardware queue instead of 572 / 520 / 520 / 520 -- but a replayed graph then puts every second successor on the same
//  second queue: 79 of 82 fast-forwards in line behind each other, 209 M env steps/s instead of 700.)
int defer_mode(const TbHandle* h);
int launch_ff(TbHandle* h, int slot, KArgs a, hipStream_t s) {
  const void *term = a.term_obs, *substeps = a.substeps;
  Pool& pool = h->pool;
  FfSlot& f = h->slots.s[slot];
  hipStream_t side = f.side;
  // lockstep episodes (every env parks in the same launch): a few envs per wave; without the host knowing the
  // phase every step is followed by this kernel and nearly every record is idle: plain 64 per wave, one flag test each
  a.ff_lanes = h->phase.valid ? h->ff_lanes : 64;
  if (int rc = fork_side(f, s)) return rc;
  // two fast-forwards that write the same terminal-obs / substeps buffer must finish in order
  if (const Slots& sl = h->slots; sl.last >= 0 && sl.last != slot && ((term && term == sl.last_term) || (substeps && substeps == sl.last_sub)))
    HIP_TRY(hipStreamWaitEvent(side, sl.s[sl.last].ev_ff, 0));
  // phases: budgeted loop + survivor kernels (see tb_ff_kernel). Without the host knowing the episode phase nearly every
  // record is idle: one plain kernel.
  const int phases = h->phase.valid ? h->ff_phases : 1;
  const bool rg = extended_contacts(h->kp);
  // deferred stragglers: on request (TbOptions.ff_defer > 0), or by default with racket<->court contact, whose resting stacks run
  // to the 800-substep limit. Not with progress marks (a mark promises that the steps before it are FINAL), not with late-written
  // terminal observations / substep counts (the pool keeps one destination per record: the reward's)
  const bool defer = pool.rec && phases == 1 && h->phase.valid && !term && !substeps && defer_mode(h) == 1;
  if (phases > 1) HIP_TRY(hipMemsetAsync(f.count, 0, 2 * sizeof(int), side));
  for (int ph = 0; ph < phases; ++ph) {
    KArgs k = a;
    dim3 grid((unsigned)((a.n + a.ff_lanes - 1) / a.ff_lanes));
    if (ph > 0) {  // survivors of phase ph: a compacted list of unknown length, walked by a fixed grid
      k.ff_rec = f.list[ph - 1]; k.ff_flag = nullptr; k.ff_src_count = f.count + (ph - 1); k.ff_lanes = TB_PHASE_LANES;
      int g = h->n / TB_PHASE_GRID_DIV; g = g < 64 ? 64 : g;  // (1 M envs, same box: / 512 9.37, / 256 9.56, / 128 9.41, / 1024 9.19 G env steps/s)
      grid = dim3((unsigned)g);
    }
    if (ph + 1 < phases) { k.ff_next = f.list[ph]; k.ff_next_count = f.count + ph; }
    if (defer) {
      // with racket<->court contact every lane is on a path of its own (rackets land at different times, manifolds of different
      // sizes, solves of different lengths) and a wave pays for the union: 16 envs per wave (4096 envs, same box: 84-86 M env
      // steps/s with 64, 92-96 with 32, 94-98 with 16, 93-97 with 8, 89 with 4)
      if (rg && !h->opt.ff_lanes_per_wave && k.ff_lanes > 16) { k.ff_lanes = 16; grid = dim3((unsigned)((a.n + 15) / 16)); }
      k.ff_next = pool.rec; k.ff_next_count = pool.count; k.ff_cap = pool.cap; k.pool_dst_out = pool.dst;
      k.ff_extra = h->opt.ff_defer_margin ? h->opt.ff_defer_margin : 16;
      pool.pending = 1;
      if (pool.run_ev_valid) HIP_TRY(hipStreamWaitEvent(side, pool.ev_run, 0));  // append behind the last pool run and its counter reset
    }
    const bool big = !defer && h->n >= 131072;  // (the deferring kernel is the small-batch POOL instantiation at any size)
    const bool esc = big && ph == 0 && phases > 1;
    if (int rc = launch_ff_kernel(rg, big, esc, defer, grid, dyn_lds(ff_lds_words(rg, esc), 64), side, k)) return rc;
  }
  return close_side(h, slot, term, substeps, s);
}

// ONE launch for what the pool holds: the whole episodes parked straight into it (ff_defer = 2) that no launch has been given to yet
// -- regions [pool_run_upto, pool_episodes): the host knows how many records -- or, without any, the stragglers that the episodes'
// own fast-forward kernels moved on to it (ff_defer = 1: their number is the pool's device counter)
int run_pool(TbHandle* h, hipStream_t q) {
  KArgs k = base_args(h);
  Pool& pool = h->pool;
  const bool rg = extended_contacts(h->kp);
  k.ff_rec = pool.rec; k.ff_flag = nullptr; k.ff_src_count = pool.count; k.ff_lanes = 64;
  k.ff_cap = (int)pool.records(); k.pool_dst_in = pool.dst;
  long long records = (long long)pool.records();
  if (pool.episodes > 0) {
    const size_t first = (size_t)pool.run_upto * h->n;
    records = (long long)(pool.episodes - pool.run_upto) * h->n;
    k.ff_src_count = nullptr; k.n = (int)records;
    k.ff_rec = pool.rec + first * pool_rec(h); k.pool_dst_in = pool.dst + first;
  }
  long long g = (records + 63) / 64;
  g = g < 1024 ? 1024 : g > 16384 ? 16384 : g;  // (workgroups beyond the pool's fill exit at once; grid-stride beyond 1 M records)
  // whole episodes in the pool make it a LARGE batch -- 43 episodes x 4096 envs = 2752 waves: the instantiation built for occupancy
  // (153 VGPRs, three waves per SIMD, wave-shared outline sweep) holds them all at once, the small-batch one (188 VGPRs, two per
  // SIMD) ran them in two rounds
  const bool big = !rg && pool.episodes > 0 && records >= 131072;
  (void)hipGetLastError();
  if (int rc = launch_ff_kernel(rg, big, false, true, dim3((unsigned)g), dyn_lds(ff_lds_words(rg, false), 64), q, k)) return rc;
  pool.run_upto = pool.episodes;
  return TB_OK;
}

// every result of every fast-forward is in place once `s` gets past this point
int flush_all(TbHandle* h, hipStream_t s) {
  if (int rc = wait_side(h, s)) return rc;
  Pool& pool = h->pool;
  if (pool.pending) {  // what the episodes since the last flush left in the pool, side by side in one launch
    if (pool.episodes > 0 && pool.direct_ev_valid) HIP_TRY(hipStreamWaitEvent(s, pool.ev_direct, 0));  // (a flush on another stream than the steps')
    if (pool.episodes == 0 || pool.run_upto < pool.episodes) {
      if (int rc = run_pool(h, s)) return rc;
    }
    HIP_TRY(hipMemsetAsync(pool.count, 0, sizeof(int), s));
    HIP_TRY(hipEventRecord(pool.ev_run, s));
    pool.idle(); pool.run_ev_valid = 1;
  }
  return TB_OK;
}

// Progress marks with ff_defer = 2: a mark promises that the steps before it are FINAL, so the episodes parked since the last mark
// (or flush) get their pool launch now -- on a side stream, beside the steps of the next chunk, counted like any fast-forward kernel.
// A graph of C chunks forks C times instead of once per episode.
int run_pool_for_mark(TbHandle* h, hipStream_t s) {
  if (!(h->pool.episodes > h->pool.run_upto)) return TB_OK;
  const int slot = h->slots.claim();
  if (int rc = fork_side(h->slots.s[slot], s)) return rc;
  if (int rc = run_pool(h, h->slots.s[slot].side)) return rc;
  return close_side(h, slot, nullptr, nullptr, s);
}

// What TbOptions.ff_defer = 0 (auto) means for this handle: 2 -- every episode end straight into the pool -- up to 16384 envs, where
// the rollout is a chain of launch-bound step kernels and every fork of a replayed graph costs the CHAIN (the next step moves to
// another hardware queue: ~10 us per episode end, and 1.7-2.8 us between all other steps instead of ~1.2 us in a graph that is one
// single list): 4096 envs, same box, 679 -> 871 M env steps/s (1024: 160 -> 225 M, 8192: 1.30 -> 1.49 G, 16384: 2.58 -> 2.63 G, 32768:
// 4.80 -> 4.26 G; racket<->court contact at 4096 envs: 92 -> 115-127 M). Above that: 1 (stragglers only) with racket<->court contact up
// to the pool's size limit, else 0 -- large batches run their fast-forwards beside the steps, in phases.
// With progress marks on, the automatic choice stays with one kernel per episode end: a graph of 8 marked chunks whose chunks are
// all-gathered beside it (one rank, 4096 envs, same box) replays in 6.3 ms that way and in 6.6-7.1 ms with the pool run at each mark
// (ff_defer = 2 asks for that); form 1 never runs under marks (a mark promises final steps).
int defer_mode(const TbHandle* h) {
  if (!h->pool.rec || h->opt.ff_defer < 0) return 0;
  if (h->opt.ff_defer > 0) return h->marks.on && h->opt.ff_defer == 1 ? 0 : h->opt.ff_defer;
  if (h->marks.on) return 0;
  if (h->n <= 16384) return 2;
  return (h->kp.flags & TB_F_RACKET_GROUND) ? 1 : 0;
}

// Where a launch that may end the episodes parks them. TbOptions.ff_defer = 2: STRAIGHT into the pool -- region [k n, (k + 1) n) for
// the k-th such launch since the last flush -- and no fast-forward kernel of its own follows: the pool run at the join does all of
// them at once (not with progress marks / late-written outputs / a full pool). Otherwise a slot, whose fast-forward follows the launch.
struct Park { bool direct; int slot; };  // into the pool, or into `slot` (-1 and not direct: the launch parks nothing)
int claim_park(TbHandle* h, bool may_park, KArgs& a, hipStream_t s, Park* p) {
  *p = Park{false, -1};
  if (!may_park) return TB_OK;
  a.defer = 1;
  Pool& pool = h->pool;
  if (pool.rec && defer_mode(h) == 2 && h->phase.valid && !a.term_obs && !a.substeps && pool.episodes < pool.cap / h->n) {
    if (pool.run_ev_valid) HIP_TRY(hipStreamWaitEvent(s, pool.ev_run, 0));  // behind the last pool run (which may have been enqueued on another stream)
    a.ff_rec = pool.rec + (size_t)pool.episodes * h->n * pool_rec(h); a.ff_flag = nullptr;
    a.pool_dst_out = pool.dst + (size_t)pool.episodes * h->n;
    p->direct = true;
    return TB_OK;
  }
  p->slot = h->slots.claim();
  const FfSlot& f = h->slots.s[p->slot];
  if (f.busy) HIP_TRY(hipStreamWaitEvent(s, f.ev_ff, 0));  // slot still in use by an older fast-forward
  a.ff_rec = f.rec; a.ff_flag = f.flag;
  return TB_OK;
}
// after the launch `a` describes: a pool region is counted (the next flush or mark runs it); a slot gets its fast-forward, which owes
// its reward to the step that parked -- the launch's last, `reward_step_stride` elements per step
int finish_park(TbHandle* h, const Park& p, KArgs a, size_t reward_step_stride, hipStream_t s) {
  if (p.direct) {
    HIP_TRY(hipEventRecord(h->pool.ev_direct, s));
    h->pool.direct_ev_valid = 1; h->pool.episodes++; h->pool.pending = 1;
    return TB_OK;
  }
  if (p.slot < 0) return TB_OK;
  a.reward += (size_t)(a.T - 1) * reward_step_stride;
  return launch_ff(h, p.slot, a, s);
}

// The substep counter's host share. Every agent step runs at least one substep of every env: n x T per launch, known to the host --
// the kernels only count what goes beyond (fast-forward loops). Added when a launch is enqueued to run; a launch that is only being
// CAPTURED runs nothing: whoever replays the graph reports the replayed steps through tb_phase_advance, as it must for the episode
// phase anyway. (tb_counters joins the stream before it reads: what was enqueued has run by then.)
int count_first_substeps(TbHandle* h, int T, hipStream_t s) {
  hipStreamCaptureStatus st;
  if (int rc = capture_status(s, &st)) return rc;
  if (st == hipStreamCaptureStatusNone) h->first_substeps += (unsigned long long)h->n * (unsigned long long)T;
  return TB_OK;
}

struct PolicyIO {  // non-null weights = fused policy step
  const float* weights; const float* obs_in; float* actions; float* raw; float* logp; float* value;
  unsigned long long seed; int deterministic;
  int net;  // TB_NET_*: checked against the env kind by policy_net_ok
  void apply(KArgs& a) const {
    a.pol_weights = weights; a.pol_obs = obs_in; a.pol_actions = actions; a.pol_raw = raw; a.pol_logp = logp;
    a.pol_value = value; a.pol_seed = seed; a.pol_deterministic = deterministic;
  }
};

// Which form of the pipelined SwingRacket one-step kernel a launch gets (tb_step_form's values). A handle with the two-wave kernel
// (TbOptions.step_waves) runs it where the variant has that form -- and the host, which knows the episode phase while the envs are in
// lockstep, picks per launch: steps 1-25 (every env has done = 0 and step_count = phase < 25) the SHORT form, whose waves load only
// their own side and test nothing before they compute; the 26th step, where every env parks, the one-wave kernel at once, without a
// ball wave started only to be thrown away; with the phase unknown (a masked reset, an injected state) the form with the early gate
// and the full loads. A captured launch keeps the form of the phase it was captured at, like its fast-forward slot.
enum { TB_STEP_ONE_WAVE = 0, TB_STEP_TWO_WAVE_GATE = 1, TB_STEP_TWO_WAVE_SHORT = 2 };
int step_form(const TbHandle* h, bool lean, bool multi, bool rg, bool policy) {
  if (!h->two_wave || !step_has_two_waves(h->kind, lean, multi, rg, policy)) return TB_STEP_ONE_WAVE;
  if (!h->phase.valid) return TB_STEP_TWO_WAVE_GATE;
  return h->phase.launch_ends_episode(1) ? TB_STEP_ONE_WAVE : TB_STEP_TWO_WAVE_SHORT;
}

// lean_multi (T > 1): the caller guarantees lockstep episodes (phase_valid) and that an episode can only
// end at the LAST of the T steps (phase + T <= 26), so the launch parks at most once per env and the
// pipelined kernel (no in-kernel fast-forward) can run several steps per launch too.
int launch_step(TbHandle* h, int T, const float* actions, float* obs, float* reward, uint8_t* done, float* term, int32_t* substeps, hipStream_t s,
                const PolicyIO* pol = nullptr, bool lean_multi = false) {
  if (int rc = count_first_substeps(h, T, s)) return rc;
  KArgs a = base_args(h);
  if (pol) pol->apply(a);
  a.actions = actions; a.obs = obs; a.reward = reward; a.done_out = done; a.term_obs = term; a.substeps = substeps; a.T = T;
  dim3 grid((unsigned)((h->n + h->block - 1) / h->block)), block((unsigned)h->block);
  if (pol) { grid = dim3((unsigned)((h->n + 63) / 64)); block = dim3(256); }  // four waves per 64 envs
  // Pipelined SwingRacket: the step kernel never loops (LEAN); a lane that starts a fast-forward is
  // parked and tb_ff_kernel finishes it on a side stream. When the host knows the episode phase (all
  // envs were reset together; episodes are exactly 26 steps) only the 26th call can park anything, so
  // only that call is followed by tb_ff_kernel; when it does not (masked reset, injected state), every
  // call gets a slot and a (then mostly idle) tb_ff_kernel.
  // With the phase known and not at the 26th step, every env has step_count = phase < 25 (all were reset
  // together and every library call that could break lockstep clears phase_valid), so no lane can start a
  // fast-forward in this launch and the lean kernel needs no slot (a.ff_rec stays null). Should the
  // invariant ever be broken, the lane is counted in counters[8] (lockstep violations) instead of being dropped silently.
  const bool piped = (T == 1 || lean_multi) && h->pipeline && h->kind == TB_ENV_SWING && (h->kp.flags & TB_F_AUTO_RESET);
  const bool may_park = piped && ((T == 1 && !h->phase.valid) || h->phase.launch_ends_episode(T));
  Park park;
  if (int rc = claim_park(h, may_park, a, s, &park)) return rc;
  const bool rg = extended_contacts(h->kp);  // selects the instantiation that contains the rolling-friction rows
  const bool multi = T > 1, policy = pol != nullptr;
  // the handle's two-wave kernel in the form the episode phase allows (step_form): the parking step of lockstep episodes goes to the
  // one-wave kernel directly, with the grid and block of a step_waves = 1 handle
  const int form = step_form(h, piped, multi, rg, policy);
  const bool two_wave = form != TB_STEP_ONE_WAVE;
  const StepKernel kern = form == TB_STEP_TWO_WAVE_SHORT ? tb_step_kernel<TB_ENV_SWING, true, false, false, false, true, TB_NET_DEFAULT, true>
                                                         : step_kernel(h->kind, piped, multi, rg, policy, two_wave, pol ? pol->net : TB_NET_DEFAULT);
  if (!kern) return fail(TB_E_UNSUPPORTED, "no tb_step_kernel instantiation for this variant");
  if (two_wave) { grid = dim3((unsigned)((h->n + 63) / 64)); block = dim3(128); }  // two waves per 64 envs
  const size_t lds = dyn_lds(step_lds_words(h->kind, piped, multi, rg, policy), policy ? 64u : block.x);
  (void)hipGetLastError();  // the check below is about THIS launch, not about whatever another library left behind
  if (int rc = launch(kern, grid, block, lds, s, a.words, a.done_state, a.actions, a.hull, a.n, a.P.n_hull, a)) return rc;
  if (int rc = finish_park(h, park, a, h->n, s)) return rc;
  h->phase.advance(T);
  return TB_OK;
}

// ---- the two host paths of the kernels that step envs in a loop with a network in front of them (tb_kernels.hpp, "THE ENV WAVE")
int refusal(int code, const char* who, const char* what) {
  char msg[320];
  snprintf(msg, sizeof msg, "%s%s", who, what);
  return fail(code, msg);
}
// the workgroups of the kernels whose env wave holds one slice of TB_POLICY_SLICE envs (their dynamic LDS: that wave's columns)
dim3 slice_groups(const TbHandle* h) { return dim3((unsigned)((h->n + TB_POLICY_SLICE - 1) / TB_POLICY_SLICE)); }
// A POPULATION over the handle's envs, n_members x envs_per_member of them, member m's floats in row m of `base`: what every entry
// point that takes one refuses. granule: the envs that share a member's weights in one workgroup (TB_POLICY_SLICE; 1 for tb_es_evaluate)
int members_refused(const char* who, const TbHandle* h, int n_members, int envs_per_member, int granule, size_t stride_floats, int min_floats, const void* base) {
  char msg[160];
  if (n_members < 1 || envs_per_member < 1 || envs_per_member % granule) {
    snprintf(msg, sizeof msg, ": n_members must be >= 1 and envs_per_member a positive multiple of the member granule (%d)", granule);
    return refusal(TB_E_INVAL, who, msg);
  }
  if ((long long)n_members * envs_per_member != h->n) return refusal(TB_E_INVAL, who, ": n_members * envs_per_member must equal n_envs");
  if (stride_floats % 4 || stride_floats < (size_t)min_floats || reinterpret_cast<uintptr_t>(base) % 16) {
    snprintf(msg, sizeof msg, ": the members' row stride must be a multiple of 4 floats and >= a member's %d, the base 16-byte aligned", min_floats);
    return refusal(TB_E_INVAL, who, msg);
  }
  return TB_OK;
}

// WHOLE EPISODES of every env, one launch (tb_es_evaluate, tb_policy_evaluate, tb_sac_evaluate; `who` names the entry point, which has
// checked its own arguments: nothing is allocated, reset or launched before this). Every env is reset, runs through its first `done`,
// and the state words are not written: on return every env is at its episode's start, phase 0, as tb_reset left it. SwingRacket's
// 26th step parks its fast-forward, whose reward goes to d_es_rew; behind the flush tb_es_fold_kernel adds it to return_dev, and to
// row 25 of a trace's reward (trace_rew, of trace_steps rows) that reaches so far. `issue(a, rg, s)` is the one kernel launch.
template <class Launch>
int run_whole_episodes(TbHandle* h, const char* who, const PolicyIO* pol, double* return_dev, int trace_steps, float* trace_rew, void* stream, Launch issue) {
  const bool swing = h->kind == TB_ENV_SWING;
  if (swing && !h->pipeline)
    return refusal(TB_E_UNSUPPORTED, who, " on SwingRacket-v0 needs tb_set_pipeline(h, 1): the 26th step's fast-forward runs on the pipeline's kernels");
  DeviceGuard g(h->device);
  hipStream_t s = (hipStream_t)stream;
  if (swing && !h->d_es_rew) HIP_TRY(hipMalloc((void**)&h->d_es_rew, sizeof(float) * (size_t)h->n));
  if (int rc = tb_reset(h, nullptr, nullptr, stream)) return rc;  // (flushes the pipeline; every env in lockstep at phase 0)
  KArgs a = base_args(h);
  if (pol) pol->apply(a);
  a.reward = h->d_es_rew;  // (SwingRacket: the fast-forward's destination for the 26th step's reward)
  Park park;
  if (int rc = claim_park(h, swing, a, s, &park)) return rc;  // (a slot for every env)
  (void)hipGetLastError();
  if (int rc = issue(a, extended_contacts(h->kp), s)) return rc;
  if (swing) {
    if (int rc = finish_park(h, park, a, 0, s)) return rc;
    if (int rc = flush_all(h, s)) return rc;  // every fast-forward's reward is in d_es_rew once `s` gets past here
    float* const last_rew = trace_steps >= kEpisodeSteps ? trace_rew : nullptr;  // (a trace that reaches the episode's last step)
    if (int rc = launch(tb_es_fold_kernel, dim3((unsigned)((h->n + 255) / 256)), dim3(256), 0, s, h->d_es_rew, return_dev, h->n, last_rew)) return rc;
  }
  return TB_OK;
}

// T STEPS FROM THE HANDLE'S STATE, one launch, episodes restarting inside it (tb_policy_rollout's launches, tb_sac_collect). What
// both refuse:
int refuse_steps_from_state(const TbHandle* h, const char* who) {
  if (!(h->kp.flags & TB_F_AUTO_RESET)) return refusal(TB_E_UNSUPPORTED, who, " needs TB_F_AUTO_RESET (episodes must restart inside the launch)");
  if (h->kind == TB_ENV_SWING && !(h->pipeline && h->phase.valid))
    return refusal(TB_E_UNSUPPORTED, who, " on SwingRacket-v0 needs tb_set_pipeline(h, 1) and episodes in lockstep (every env reset together): "
                                          "the fast-forward that ends an episode cannot run inside a multi-step launch");
  return TB_OK;
}
// SwingRacket: the caller keeps T inside the episode, so only a launch that ends where the episodes do parks anything; the parked
// step's reward goes to row T - 1 of a.reward (rows reward_step_stride apart). `issue(a, rg)` is the one kernel launch. flush: every
// output, the terminal reward included, is in place once `s` gets past the call.
template <class Launch>
int run_steps_from_state(TbHandle* h, int T, KArgs a, size_t reward_step_stride, bool flush, hipStream_t s, Launch issue) {
  if (int rc = count_first_substeps(h, T, s)) return rc;
  const bool swing = h->kind == TB_ENV_SWING;
  const bool may_park = swing && h->phase.launch_ends_episode(T);
  Park park;
  if (int rc = claim_park(h, may_park, a, s, &park)) return rc;
  (void)hipGetLastError();
  if (int rc = issue(a, extended_contacts(h->kp))) return rc;
  if (int rc = finish_park(h, park, a, reward_step_stride, s)) return rc;
  if (flush && swing) {
    if (int rc = flush_all(h, s)) return rc;
  }
  h->phase.advance(T);
  return TB_OK;
}

// one launch of tb_policy_rollout_kernel over T steps; SwingRacket: T ends where the episode does. members: null, or the population
// whose blobs pol.weights holds (the kernel's members form: the same grid, block and LDS)
int launch_policy_rollout(TbHandle* h, int T, const PolicyIO& pol, float* obs, float* reward, uint8_t* done, const size_t* st /*element strides*/,
                          hipStream_t s, const PolicyMembers* members = nullptr) {
  KArgs a = base_args(h);
  pol.apply(a);
  a.obs = obs; a.reward = reward; a.done_out = done; a.T = T;
  a.st_act = st[0]; a.st_raw = st[1]; a.st_logp = st[2]; a.st_val = st[3]; a.st_obs = st[4]; a.st_rew = st[5]; a.st_done = st[6];
  return run_steps_from_state(h, T, a, st[5], false, s, [&](const KArgs& k, bool rg) {
    // 16 envs per workgroup (3 waves) while every workgroup still gets a CU of its own, else 48 (7 waves): see the kernel
    const bool narrow = h->opt.policy_slices ? h->opt.policy_slices == 1 : h->n <= 4096;
    const int E = narrow ? TB_POLICY_SLICE : 3 * TB_POLICY_SLICE;
    if (members) {
      using MembersKernel = void (*)(KArgs, PolicyMembers);
      const MembersKernel kern = kernel_of_kind_net_rg(h->kind, pol.net, rg, [&](auto K, auto N, auto R) -> MembersKernel {
        return narrow ? tb_policy_rollout_kernel<K.value, 1, R.value, N.value, PolicyMembers> : tb_policy_rollout_kernel<K.value, 3, R.value, N.value, PolicyMembers>;
      });
      if (!kern) return fail(TB_E_UNSUPPORTED, "no tb_policy_rollout_kernel members instantiation for this variant");
      return launch(kern, dim3((unsigned)((h->n + E - 1) / E)), dim3(narrow ? 192 : 448), dyn_lds(policy_rollout_lds_words(h->kind, rg), 64), s, k, *members);
    }
    const ArgsKernel kern = kernel_of_kind_net_rg(h->kind, pol.net, rg, [&](auto K, auto N, auto R) -> ArgsKernel {
      return narrow ? tb_policy_rollout_kernel<K.value, 1, R.value, N.value> : tb_policy_rollout_kernel<K.value, 3, R.value, N.value>;
    });
    if (!kern) return fail(TB_E_UNSUPPORTED, "no tb_policy_rollout_kernel instantiation for this variant");
    return launch(kern, dim3((unsigned)((h->n + E - 1) / E)), dim3(narrow ? 192 : 448), dyn_lds(policy_rollout_lds_words(h->kind, rg), 64), s, k);  // (the env wave's columns)
  });
}

// every fast-forward's result in place, then `bytes` of device memory read back; the host has them on return
int read_back(TbHandle* h, void* dst, const void* src_dev, size_t bytes, hipStream_t s) {
  if (int rc = flush_all(h, s)) return rc;
  HIP_TRY(hipMemcpyAsync(dst, src_dev, bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return TB_OK;
}

// tb_set_state with the pipeline on: the pipelined kernels need to know which launch ends the episodes. The injected envs are in
// lockstep again when every one is running (done = 0) at the same step count below the episode length -- then the phase is that
// count (e.g. a checkpoint of a training run restored into a fresh handle). Costs one small device-to-host copy and a stream
// synchronisation (so: not capturable, and not asynchronous even with on_device); only paid with the pipeline on,
// the one mode that uses the phase -- without it the call stays fully asynchronous for on_device buffers.
int rederive_phase(TbHandle* h, hipStream_t s) {
  const size_t n = (size_t)h->n;
  uint32_t* steps = (uint32_t*)malloc(n * sizeof(uint32_t));
  uint8_t* dn = (uint8_t*)malloc(n);
  if (!steps || !dn) { free(steps); free(dn); return fail(TB_E_INVAL, "tb_set_state: out of host memory"); }
  hipError_t e = hipMemcpyAsync(steps, h->d_words + (size_t)TB_W_SW_STEP * n, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(dn, h->d_done, n, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e == hipSuccess) {
    bool same = (int32_t)steps[0] >= 0 && (int32_t)steps[0] < kEpisodeSteps;
    for (size_t i = 0; same && i < n; ++i) same = steps[i] == steps[0] && dn[i] == TB_DONE_NO;
    if (same) h->phase.set((int)steps[0]);
  }
  free(steps); free(dn);
  return e == hipSuccess ? TB_OK : fail((int)e, "tb_set_state: reading back the step counters");
}

// the pipeline's streams, events and buffers: all of them, or none (what release_pipeline leaves behind is the state of a
// handle whose pipeline was never enabled)
void release_pipeline(TbHandle* h) {
  for (FfSlot& f : h->slots.s) { f.free_buffers(); f.close(); }
  h->pool.release();
  h->pipeline = 0;
}

int alloc_pool(TbHandle* h, uint32_t flags) {  // all of it or none: defer_mode takes a non-null pool.rec for a usable pool
  if (h->pool.rec || h->n > TB_DEFER_MAX_ENVS || h->opt.ff_defer < 0) return TB_OK;
  if (!(h->opt.ff_defer > 0 || h->n <= 16384 || (flags & TB_F_RACKET_GROUND))) return TB_OK;  // (see Pool: who can ever defer)
  Pool p = {};
  if (int rc = p.build(h->n)) { p.release(); return rc; }
  h->pool = p;
  return TB_OK;
}

int alloc_pipeline(TbHandle* h) {
  for (FfSlot& f : h->slots.s)
    if (int rc = f.build(h->n, h->ff_phases)) return rc;
  if (int rc = alloc_pool(h, h->kp.flags)) return rc;
  HIP_TRY(hipDeviceSynchronize());
  return TB_OK;
}

}  // namespace

extern "C" {

int tb_abi_version(void) { return TB_ABI_VERSION; }
int tb_obs_dim(int k) { return k == TB_ENV_SWING ? TB_SWING_OBS_DIM : k == TB_ENV_TENNIS ? TB_TENNIS_OBS_DIM : TB_E_INVAL; }
int tb_act_dim(int k) { return k == TB_ENV_SWING ? TB_SWING_ACT_DIM : k == TB_ENV_TENNIS ? TB_TENNIS_ACT_DIM : TB_E_INVAL; }
int tb_state_words(int k) { return kind_ok(k) ? words_of(k) : TB_E_INVAL; }
const char* tb_last_error(void) { return g_err; }

int tb_create(const TbParams* params, const TbOptions* options, int env_kind, int n_envs, int device, uint64_t seed, uint64_t env_id_base, TbHandle** out) {
  if (!params || !out) return fail(TB_E_INVAL, "tb_create: null argument");
  *out = nullptr;
  if (!kind_ok(env_kind)) return fail(TB_E_INVAL, "tb_create: unknown env kind");
  if (n_envs <= 0 || n_envs > (1 << 25)) return fail(TB_E_INVAL, "tb_create: n_envs must be in [1, 2^25]");  // (32-bit row offsets: see row_word)
  if (int rc = validate_params(params)) return rc;
  TbOptions opt;
  memset(&opt, 0, sizeof opt);
  if (options) {  // a caller built against an older (shorter) TbOptions leaves the newer fields at "auto"
    if (options->struct_size < sizeof(uint32_t) || options->struct_size > 4096) return fail(TB_E_INVAL, "tb_create: TbOptions.struct_size is not set");
    memcpy(&opt, options, options->struct_size < sizeof opt ? options->struct_size : sizeof opt);
    if (opt.block != 0 && opt.block != 64 && opt.block != 128 && opt.block != 256) return fail(TB_E_INVAL, "tb_create: TbOptions.block must be 0, 64, 128 or 256");
    if (opt.ff_lanes_per_wave < 0 || opt.ff_lanes_per_wave > 64) return fail(TB_E_INVAL, "tb_create: TbOptions.ff_lanes_per_wave must be in [0, 64]");
    if (opt.ff_phases < 0 || opt.ff_phases > 3) return fail(TB_E_INVAL, "tb_create: TbOptions.ff_phases must be in [0, 3]");
    if (opt.policy_slices != 0 && opt.policy_slices != 1 && opt.policy_slices != 3) return fail(TB_E_INVAL, "tb_create: TbOptions.policy_slices must be 0, 1 or 3");
    if (opt.ff_defer < -1 || opt.ff_defer > 2) return fail(TB_E_INVAL, "tb_create: TbOptions.ff_defer must be -1, 0, 1 or 2");
    if (opt.ff_defer_margin < 0 || opt.ff_defer_margin > 800) return fail(TB_E_INVAL, "tb_create: TbOptions.ff_defer_margin must be in [0, 800]");
    if (opt.ff_seal < -1 || opt.ff_seal > 1) return fail(TB_E_INVAL, "tb_create: TbOptions.ff_seal must be -1, 0 or 1");
    if (opt.step_waves < 0 || opt.step_waves > 2) return fail(TB_E_INVAL, "tb_create: TbOptions.step_waves must be 0, 1 or 2");
  }
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0) return fail(TB_E_NODEVICE, "tb_create: no HIP device available (this library has no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(TB_E_NODEVICE, "tb_create: device index out of range");
  DeviceGuard g(device);
  if (g.err != hipSuccess) return fail((int)g.err, "hipSetDevice");

  TbHandle* h = (TbHandle*)calloc(1, sizeof(TbHandle));
  if (!h) return fail(TB_E_INVAL, "tb_create: out of host memory");
  h->device = device; h->kind = env_kind; h->n = n_envs; h->seed = seed; h->env_id_base = env_id_base;
  h->params = *params; to_kparams(params, &h->kp, &h->cull_planes[0][0]); h->block = pick_block(env_kind, n_envs, opt);
  h->opt = opt;
  // two waves per 64 envs where SIMDs are idle anyway: 4096 envs, same box, see profiles/r05_two_wave_ab.txt
  h->two_wave = opt.step_waves ? opt.step_waves == 2 : n_envs <= TB_TWO_WAVE_MAX_ENVS;
  // measured on one box: 3 phases +11 % at 1 M envs, +-0 at 256 K, -16 % at 32 K and 4096 (two more kernels in every episode's chain)
  h->ff_phases = opt.ff_phases >= 1 && opt.ff_phases <= 3 ? opt.ff_phases : (n_envs >= 262144 ? 3 : 1);
  h->ff_lanes = opt.ff_lanes_per_wave;  // fast-forward: 64 envs per wave from 4096 envs on, a few per wave below
  if (!h->ff_lanes) { h->ff_lanes = 4; while (h->ff_lanes < 64 && (long long)h->ff_lanes * 64 < n_envs) h->ff_lanes <<= 1; }
  const int nw = words_of(env_kind);
  hipError_t err;
#define CREATE_TRY(expr) if ((err = (expr)) != hipSuccess) { int rc = fail((int)err, #expr); tb_destroy(h); return rc; }
  CREATE_TRY(hipMalloc((void**)&h->d_words, sizeof(uint32_t) * (size_t)nw * n_envs));
  CREATE_TRY(hipMalloc((void**)&h->d_done, (size_t)n_envs));
  CREATE_TRY(hipMalloc((void**)&h->d_hull, sizeof(float4) * TB_HULL_LDS));
  CREATE_TRY(hipHostMalloc((void**)&h->h_hull, sizeof(float4) * TB_HULL_LDS, hipHostMallocDefault));
  CREATE_TRY(hipMalloc((void**)&h->d_counters, sizeof(unsigned long long) * kCounterWords));
  CREATE_TRY(hipMemsetAsync(h->d_counters, 0, sizeof(unsigned long long) * kCounterWords, 0));
  CREATE_TRY(hipMalloc((void**)&h->d_mani, sizeof(uint32_t) * (size_t)TB_MANI_WORDS * n_envs));
  CREATE_TRY(hipMalloc((void**)&h->d_mflag, (size_t)n_envs));
  CREATE_TRY(hipMemsetAsync(h->d_mflag, 0, (size_t)n_envs, 0));
  if (int rc = launch(tb_init_kernel, dim3((unsigned)((n_envs + 255) / 256)), dim3(256), 0, 0, h->d_words, h->d_done, n_envs, nw)) { tb_destroy(h); return rc; }
  if (int rc = upload_hull(h, 0)) { tb_destroy(h); return rc; }
  CREATE_TRY(hipStreamSynchronize(0));
#undef CREATE_TRY
  *out = h;
  return TB_OK;
}

int tb_destroy(TbHandle* h) {
  if (!h) return TB_OK;
  DeviceGuard g(h->device);
  (void)hipDeviceSynchronize();
  drop(h->d_words); drop(h->d_done); drop(h->d_hull); drop(h->d_counters); drop(h->d_mani); drop(h->d_mflag); drop(h->d_es_rew);
  if (h->h_hull) (void)hipHostFree(h->h_hull);
  release_pipeline(h);
  if (h->marks.h) (void)hipHostFree(h->marks.h);
  free(h);
  return TB_OK;
}

int tb_set_pipeline(TbHandle* h, int enable) {
  if (!h) return fail(TB_E_INVAL, "tb_set_pipeline: null handle");
  DeviceGuard g(h->device);
  if (enable && !h->slots.built()) {
    if (h->kind != TB_ENV_SWING) return fail(TB_E_UNSUPPORTED, "tb_set_pipeline: only SwingRacket-v0 has a fast-forward to overlap");
    // 8 slots x (records + up to two survivor lists) x 192 B per env: 4.6 KB per env, 77 GB at the cap (of 288)
    if (h->n > TB_PIPELINE_MAX_ENVS) return fail(TB_E_INVAL, "tb_set_pipeline: more than 2^24 envs (the parked-record slots would not fit next to the state)");
    h->slots.forget_ordering();
    if (int rc = alloc_pipeline(h)) {
      // all or nothing: a half-built pipeline would pass the `built()` test above on the next call and the step kernel would
      // then park into a null slot. fail() has already recorded what went wrong.
      release_pipeline(h);
      (void)hipGetLastError();
      return rc;
    }
  }
  h->pipeline = enable ? 1 : 0;
  return TB_OK;
}

int tb_diag_fail_alloc(int nth) {
  g_fail_alloc_countdown = nth > 0 ? nth : 0;
  return TB_OK;
}

int tb_pipeline_sync(TbHandle* h, int host_wait) {
  if (!h) return fail(TB_E_INVAL, "tb_pipeline_sync: null handle");
  DeviceGuard g(h->device);
  if (host_wait) {
    for (FfSlot& f : h->slots.s)
      if (f.side) HIP_TRY(hipStreamSynchronize(f.side));
    h->slots.forget_capture();
    h->phase.save_for_capture();
  } else h->phase.restore();  // the captured tb_step calls advanced the host's episode phase, but none of them ran: the replays will (tb_phase_advance)
  h->slots.forget_ordering();
  h->pool.events_forgotten();
  return TB_OK;
}

int tb_pipeline_recover(TbHandle* h) {
  if (!h) return fail(TB_E_INVAL, "tb_pipeline_recover: null handle");
  DeviceGuard g(h->device);
  (void)hipGetLastError();  // the abandoned capture leaves a sticky hipErrorStreamCaptureInvalidated behind
  h->phase.restore();  // the captured tb_step calls advanced the host's episode phase, but none of them ran
  h->pool.events_forgotten();
  h->pool.idle();  // episode ends that the abandoned capture "parked" into the pool never ran: nothing is pending on their account
  h->slots.forget_ordering();
  h->slots.forget_capture();  // nothing of the abandoned capture will ever run
  for (FfSlot& f : h->slots.s) {
    if (!f.side) continue;
    // a side stream that was forked into the capture stays invalidated: replace it and its events
    f.close();
    (void)hipGetLastError();
    if (int rc = f.open()) return rc;
  }
  return TB_OK;
}

int tb_flush(TbHandle* h, void* stream) {
  if (!h) return fail(TB_E_INVAL, "tb_flush: null handle");
  DeviceGuard g(h->device);
  return flush_all(h, (hipStream_t)stream);
}

int tb_phase(TbHandle* h) {
  if (!h) return fail(TB_E_INVAL, "tb_phase: null handle");
  return h->phase.valid ? h->phase.at : -1;
}

int tb_pipeline_form(TbHandle* h) {
  if (!h) return fail(TB_E_INVAL, "tb_pipeline_form: null handle");
  if (h->kind != TB_ENV_SWING || !h->pipeline) return 0;
  const int mode = defer_mode(h);
  return mode == 2 ? 3 : mode == 1 && h->ff_phases == 1 ? 2 : 1;
}

int tb_step_waves(TbHandle* h) {
  if (!h) return fail(TB_E_INVAL, "tb_step_waves: null handle");
  if (h->kind != TB_ENV_SWING || !h->pipeline) return 0;
  return h->two_wave ? 2 : 1;
}

int tb_step_form(TbHandle* h) {
  if (!h) return fail(TB_E_INVAL, "tb_step_form: null handle");
  if (h->kind != TB_ENV_SWING || !h->pipeline || !(h->kp.flags & TB_F_AUTO_RESET)) return -1;
  return step_form(h, true, false, extended_contacts(h->kp), false);
}

int tb_phase_advance(TbHandle* h, int n_steps) {
  if (!h || n_steps < 0) return fail(TB_E_INVAL, "tb_phase_advance: bad argument");
  h->phase.advance(n_steps);
  h->first_substeps += (unsigned long long)h->n * (unsigned long long)n_steps;  // the replayed steps' share of the substep counter
  return TB_OK;
}

int tb_mark_record(TbHandle* h, int k, void* stream) {
  if (!h || k < 0 || k >= TB_MAX_MARKS) return fail(TB_E_INVAL, "tb_mark_record: bad handle or mark index");
  DeviceGuard g(h->device);
  hipStream_t s = (hipStream_t)stream;
  if (!h->marks.on) return fail(TB_E_UNSUPPORTED, "tb_mark_record needs tb_mark_enable(h, 1) before the steps it covers (their fast-forwards must be counted)");
  hipStreamCaptureStatus st;
  if (int rc = capture_status(s, &st)) return rc;
  if (int rc = run_pool_for_mark(h, s)) return rc;  // (counted among the fast-forwards enqueued before the mark)
  if (int rc = launch(tb_mark_kernel, dim3(1), dim3(1), 0, s, h->marks.h + k)) return rc;
  h->marks.in_capture[k] = st == hipStreamCaptureStatusActive;
  for (int q = 0; q < TB_FF_SLOTS; ++q) h->marks.ff_before[k][q] = h->marks.in_capture[k] ? h->slots.s[q].in_capture : h->slots.s[q].eager;
  return TB_OK;
}

int tb_mark_enable(TbHandle* h, int on) {
  if (!h) return fail(TB_E_INVAL, "tb_mark_enable: null handle");
  if (on) { if (int rc = h->marks.ensure()) return rc; }
  h->marks.on = on ? 1 : 0;
  return TB_OK;
}

int tb_mark_begin(TbHandle* h) {
  if (!h) return fail(TB_E_INVAL, "tb_mark_begin: null handle");
  if (int rc = h->marks.ensure()) return rc;
  for (int q = 0; q < TB_FF_SLOTS; ++q) { h->marks.snap_ff[q] = __atomic_load_n(h->marks.h + TB_MAX_MARKS + q, __ATOMIC_ACQUIRE); h->slots.s[q].eager = 0; }
  for (int k = 0; k < TB_MAX_MARKS; ++k) h->marks.snap_marks[k] = __atomic_load_n(h->marks.h + k, __ATOMIC_ACQUIRE);
  return TB_OK;
}

long long tb_mark_count(TbHandle* h, int k) {
  if (!h || k < 0 || k >= TB_MAX_MARKS) return fail(TB_E_INVAL, "tb_mark_count: bad handle or mark index");
  if (!h->marks.h) return 0;
  return (long long)__atomic_load_n(h->marks.h + k, __ATOMIC_ACQUIRE);
}

int tb_mark_host_wait(TbHandle* h, int k, int timeout_ms) {
  if (!h || k < 0 || k >= TB_MAX_MARKS || !h->marks.h) return fail(TB_E_INVAL, "tb_mark_host_wait: bad handle, mark index, or no mark recorded yet");
  // fired once more than at tb_mark_begin, and every fast-forward enqueued before the mark has finished: those of the
  // graph that holds it (counted at capture time) plus whatever was launched eagerly since (over-waiting at worst)
  unsigned long long ff_target[TB_FF_SLOTS];
  for (int q = 0; q < TB_FF_SLOTS; ++q)
    ff_target[q] = h->marks.snap_ff[q] + (unsigned long long)(h->marks.in_capture[k] ? h->marks.ff_before[k][q] + h->slots.s[q].eager : h->marks.ff_before[k][q]);
  const unsigned long long count = h->marks.snap_marks[k] + 1;
  const auto t0 = std::chrono::steady_clock::now();
  for (unsigned spins = 0;; ++spins) {
    bool ok = __atomic_load_n(h->marks.h + k, __ATOMIC_ACQUIRE) >= count;
    for (int q = 0; ok && q < TB_FF_SLOTS; ++q) ok = __atomic_load_n(h->marks.h + TB_MAX_MARKS + q, __ATOMIC_ACQUIRE) >= ff_target[q];
    if (ok) return TB_OK;
    if ((spins & 1023u) == 1023u &&
        std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count() > timeout_ms)
      return fail(TB_E_TIMEOUT, "tb_mark_host_wait: the mark did not fire in time");
    __builtin_ia32_pause();
  }
}

int tb_set_params(TbHandle* h, const TbParams* params, void* stream) {
  if (!h || !params) return fail(TB_E_INVAL, "tb_set_params: null argument");
  if (int rc = validate_params(params)) return rc;
  DeviceGuard g(h->device);
  hipStream_t s = (hipStream_t)stream;
  // the staging buffer may still feed an earlier async copy on another stream: settle it first
  if (int rc = flush_all(h, s)) return rc;
  HIP_TRY(hipStreamSynchronize(s));
  KParams kp = h->kp;  // (what to_kparams leaves alone stays as it was)
  float planes[TB_N_CULL][3];
  to_kparams(params, &kp, &planes[0][0]);
  // Nothing in flight and nothing parked from here on. The pool first, so that a failure leaves the handle as it was: a pipelined
  // handle whose new parameter block asks for one (racket<->court contact above 16384 envs) gets it now; one that has it and
  // switches the contact set, and with it the record stride (pool_rec), starts from a zeroed pool -- no tag word of one stride can
  // land on the payload of a record of the other.
  if (h->slots.built() && !h->pool.rec) {
    if (int rc = alloc_pool(h, params->flags)) { (void)hipGetLastError(); return rc; }
    HIP_TRY(hipDeviceSynchronize());
  } else if (h->pool.rec && extended_contacts(kp) != extended_contacts(h->kp)) {
    HIP_TRY(hipMemsetAsync(h->pool.rec, 0, sizeof(float4) * (size_t)TB_FF_REC_MAX * h->pool.records(), s));
  }
  if ((params->flags ^ h->params.flags) & TB_F_AUTO_RESET) h->phase.invalidate();  // episodes may stop / start restarting
  h->params = *params; h->kp = kp;
  memcpy(h->cull_planes, planes, sizeof planes);
  if (int rc = upload_hull(h, s)) return rc;
  HIP_TRY(hipStreamSynchronize(s));
  h->params_generation++;
  return TB_OK;
}

int tb_params_generation(TbHandle* h) {
  if (!h) return fail(TB_E_INVAL, "tb_params_generation: null handle");
  return h->params_generation;
}

int tb_set_racket_scale(TbHandle* h, float scale, void* stream) {
  if (!h) return fail(TB_E_INVAL, "tb_set_racket_scale: null handle");
  if (!(scale > 0.0f)) return fail(TB_E_PARAMS, "tb_set_racket_scale: scale must be positive");
  DeviceGuard g(h->device);
  h->params.racket_scale = scale; h->kp.racket_scale = scale;  // what a later tb_set_params re-uploads
  float* dst = reinterpret_cast<float*>(h->d_hull + TB_HULL_KP) + offsetof(KParams, racket_scale) / sizeof(float);
  return launch(tb_poke_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, dst, scale);
}

int tb_reset(TbHandle* h, const uint8_t* mask_dev, float* obs_dev, void* stream) {
  if (!h) return fail(TB_E_INVAL, "tb_reset: null handle");
  DeviceGuard g(h->device);
  if (int rc = flush_all(h, (hipStream_t)stream)) return rc;
  if (mask_dev) h->phase.invalidate();  // episodes are no longer in lockstep
  else h->phase.set(0);
  KArgs a = base_args(h);
  a.mask = mask_dev; a.obs = obs_dev;
  dim3 grid((unsigned)((h->n + 255) / 256)), block(256);
  return launch(h->kind == TB_ENV_SWING ? tb_reset_kernel<TB_ENV_SWING> : tb_reset_kernel<TB_ENV_TENNIS>, grid, block, 0, (hipStream_t)stream, a);
}

int tb_step(TbHandle* h, const float* actions_dev, float* obs_dev, float* reward_dev, uint8_t* done_dev, float* terminal_obs_dev,
            int32_t* substeps_dev, void* stream) {
  if (!h || !actions_dev || !obs_dev || !reward_dev || !done_dev) return fail(TB_E_INVAL, "tb_step: null argument");
  DeviceGuard g(h->device);
  return launch_step(h, 1, actions_dev, obs_dev, reward_dev, done_dev, terminal_obs_dev, substeps_dev, (hipStream_t)stream);
}

int tb_step_sequence(TbHandle* h, int n_steps, const float* actions_dev, float* obs_dev, float* reward_dev, uint8_t* done_dev,
                     size_t actions_stride, size_t obs_stride, size_t reward_stride, size_t done_stride, void* stream) {
  if (!h || !actions_dev || !obs_dev || !reward_dev || !done_dev) return fail(TB_E_INVAL, "tb_step_sequence: null argument");
  if (n_steps < 1) return fail(TB_E_INVAL, "tb_step_sequence: n_steps must be >= 1");
  DeviceGuard g(h->device);
  for (int t = 0; t < n_steps; ++t) {
    const size_t k = (size_t)t;
    if (int rc = launch_step(h, 1, reinterpret_cast<const float*>(reinterpret_cast<const char*>(actions_dev) + k * actions_stride),
                             reinterpret_cast<float*>(reinterpret_cast<char*>(obs_dev) + k * obs_stride),
                             reinterpret_cast<float*>(reinterpret_cast<char*>(reward_dev) + k * reward_stride), done_dev + k * done_stride, nullptr, nullptr,
                             (hipStream_t)stream))
      return rc;
  }
  return TB_OK;
}

int tb_policy_floats(int env_kind) {
  return env_kind == TB_ENV_SWING ? policy_floats<TB_ENV_SWING>() : env_kind == TB_ENV_TENNIS ? policy_floats<TB_ENV_TENNIS>() : TB_E_INVAL;
}

namespace {
// is (kind, net) a pair the policy kernels are built for (with_kind_net's table)? `who`'s refusal if not
int policy_net_ok(int env_kind, int net, const char* who) {
  if (with_kind_net(env_kind, net, false, [](auto, auto) { return true; })) return TB_OK;
  char msg[256];
  if (net == TB_NET_MLP64 && env_kind == TB_ENV_TENNIS)
    snprintf(msg, sizeof msg, "%s: TB_NET_MLP64 is SwingRacket-v0's; on Tennisbot-v0 TB_NET_DEFAULT is that net (pi = vf = [64, 64], tanh)", who);
  else
    snprintf(msg, sizeof msg, "%s: net %d is not built for env kind %d (TB_NET_TUNED is Tennisbot-v0's, TB_NET_MLP64 SwingRacket-v0's; every kind has TB_NET_DEFAULT)", who,
             net, env_kind);
  return fail(TB_E_PARAMS, msg);
}
// the TRPO kernels': the above without the tuned network (its shared extractor has no instantiation of them)
int trpo_net_ok(int env_kind, int net, const char* who) {
  if (net == TB_NET_TUNED) {
    char msg[160];
    snprintf(msg, sizeof msg, "%s: TB_NET_TUNED is not built for the TRPO kernels (TB_NET_DEFAULT, or TB_NET_MLP64 on SwingRacket-v0)", who);
    return fail(TB_E_PARAMS, msg);
  }
  return policy_net_ok(env_kind, net, who);
}
}  // namespace

int tb_policy_blob_floats(int env_kind, int net) {
  if (!kind_ok(env_kind)) return TB_E_INVAL;
  if (int rc = policy_net_ok(env_kind, net, "tb_policy_blob_floats")) return rc;
  return with_kind_net(env_kind, net, 0, [](auto K, auto N) { return (int)PolicyBlob<K.value, N.value>::TOTAL; });
}

int tb_policy_step_net(TbHandle* h, int net, const float* weights_dev, const float* obs_in_dev, float* actions_dev, float* raw_actions_dev, float* logp_dev,
                       float* value_dev, float* obs_dev, float* reward_dev, uint8_t* done_dev, uint64_t noise_seed, int deterministic, void* stream) {
  if (!h || !weights_dev || !obs_in_dev || !actions_dev || !raw_actions_dev || !logp_dev || !value_dev || !obs_dev || !reward_dev || !done_dev)
    return fail(TB_E_INVAL, "tb_policy_step: null argument");
  if (int rc = policy_net_ok(h->kind, net, "tb_policy_step")) return rc;
  DeviceGuard g(h->device);
  PolicyIO pol = {weights_dev, obs_in_dev, actions_dev, raw_actions_dev, logp_dev, value_dev, noise_seed, deterministic, net};
  return launch_step(h, 1, nullptr, obs_dev, reward_dev, done_dev, nullptr, nullptr, (hipStream_t)stream, &pol);
}
int tb_policy_step(TbHandle* h, const float* weights_dev, const float* obs_in_dev, float* actions_dev, float* raw_actions_dev, float* logp_dev,
                   float* value_dev, float* obs_dev, float* reward_dev, uint8_t* done_dev, uint64_t noise_seed, int deterministic, void* stream) {
  return tb_policy_step_net(h, TB_NET_DEFAULT, weights_dev, obs_in_dev, actions_dev, raw_actions_dev, logp_dev, value_dev, obs_dev, reward_dev, done_dev, noise_seed,
                            deterministic, stream);
}

int tb_policy_rollout(TbHandle* h, int n_steps, const float* weights_dev, const float* obs_in_dev, float* actions_dev, float* raw_actions_dev,
                      float* logp_dev, float* value_dev, float* obs_dev, float* reward_dev, uint8_t* done_dev, const size_t* step_strides_bytes,
                      uint64_t noise_seed, int deterministic, void* stream) {
  return tb_policy_rollout_net(h, TB_NET_DEFAULT, n_steps, weights_dev, obs_in_dev, actions_dev, raw_actions_dev, logp_dev, value_dev, obs_dev, reward_dev, done_dev,
                               step_strides_bytes, noise_seed, deterministic, stream);
}
namespace {
// tb_policy_rollout_net and tb_policy_rollout_members (`who`; members: null, or the population -- n_members is only checked here)
int policy_rollout(const char* who, TbHandle* h, int net, int n_steps, const float* weights_dev, const PolicyMembers* members, int n_members,
                   const float* obs_in_dev, float* actions_dev, float* raw_actions_dev, float* logp_dev, float* value_dev, float* obs_dev, float* reward_dev,
                   uint8_t* done_dev, const size_t* step_strides_bytes, uint64_t noise_seed, int deterministic, void* stream) {
  if (!h || !weights_dev || !obs_in_dev || !actions_dev || !raw_actions_dev || !logp_dev || !value_dev || !obs_dev || !reward_dev || !done_dev)
    return refusal(TB_E_INVAL, who, ": null argument");
  if (n_steps < 1) return refusal(TB_E_INVAL, who, ": n_steps must be >= 1");
  if (int rc = policy_net_ok(h->kind, net, who)) return rc;
  if (members) {
    if (int rc = members_refused(who, h, n_members, members->per_member, TB_POLICY_SLICE, members->stride, tb_policy_blob_floats(h->kind, net), weights_dev)) return rc;
  }
  if (int rc = refuse_steps_from_state(h, who)) return rc;
  const bool swing = h->kind == TB_ENV_SWING;
  const size_t n = (size_t)h->n, A = swing ? TB_SWING_ACT_DIM : TB_TENNIS_ACT_DIM, O = swing ? TB_SWING_OBS_DIM : TB_TENNIS_OBS_DIM;
  size_t st[7] = {n * A, n * A, n, n, n * O, n, n};  // elements per step: actions, raw, logp, value, obs, reward, done
  if (step_strides_bytes) {
    for (int k = 0; k < 7; ++k) {
      const size_t el = k == 6 ? 1 : sizeof(float);
      if (step_strides_bytes[k] % el) return refusal(TB_E_INVAL, who, ": a step stride is not a multiple of its element size");
      if (step_strides_bytes[k]) st[k] = step_strides_bytes[k] / el;
    }
  }
  // action rows are written 8 bytes at a time (like the action rows tb_step reads): bases and step strides must keep them aligned
  if ((reinterpret_cast<uintptr_t>(actions_dev) | reinterpret_cast<uintptr_t>(raw_actions_dev)) % 8 || (st[0] * sizeof(float)) % 8 || (st[1] * sizeof(float)) % 8)
    return refusal(TB_E_INVAL, who, ": actions / raw_actions and their step strides must be 8-byte aligned");
  DeviceGuard g(h->device);
  hipStream_t s = (hipStream_t)stream;
  const float* obs_in = obs_in_dev;
  for (int t = 0; t < n_steps;) {
    const int chunk = swing ? h->phase.chunk(n_steps - t) : n_steps - t;
    PolicyIO pol = {weights_dev, obs_in, actions_dev + (size_t)t * st[0], raw_actions_dev + (size_t)t * st[1], logp_dev + (size_t)t * st[2],
                    value_dev + (size_t)t * st[3], noise_seed, deterministic, net};
    if (int rc = launch_policy_rollout(h, chunk, pol, obs_dev + (size_t)t * st[4], reward_dev + (size_t)t * st[5], done_dev + (size_t)t * st[6], st, s, members)) return rc;
    t += chunk;
    obs_in = obs_dev + (size_t)(t - 1) * st[4];  // the next launch acts on what this one observed last
  }
  return TB_OK;
}
}  // namespace
int tb_policy_rollout_net(TbHandle* h, int net, int n_steps, const float* weights_dev, const float* obs_in_dev, float* actions_dev, float* raw_actions_dev,
                          float* logp_dev, float* value_dev, float* obs_dev, float* reward_dev, uint8_t* done_dev, const size_t* step_strides_bytes,
                          uint64_t noise_seed, int deterministic, void* stream) {
  return policy_rollout("tb_policy_rollout", h, net, n_steps, weights_dev, nullptr, 0, obs_in_dev, actions_dev, raw_actions_dev, logp_dev, value_dev, obs_dev,
                        reward_dev, done_dev, step_strides_bytes, noise_seed, deterministic, stream);
}
// a population's collect: the same launches with the kernel's members form
int tb_policy_rollout_members(TbHandle* h, int net, int n_steps, const float* weights_dev, int n_members, size_t weights_stride_floats, int envs_per_member,
                              const float* obs_in_dev, float* actions_dev, float* raw_actions_dev, float* logp_dev, float* value_dev, float* obs_dev,
                              float* reward_dev, uint8_t* done_dev, const size_t* step_strides_bytes, uint64_t noise_seed, int deterministic, void* stream) {
  const PolicyMembers members = {weights_stride_floats, envs_per_member};
  return policy_rollout("tb_policy_rollout_members", h, net, n_steps, weights_dev, &members, n_members, obs_in_dev, actions_dev, raw_actions_dev, logp_dev, value_dev,
                        obs_dev, reward_dev, done_dev, step_strides_bytes, noise_seed, deterministic, stream);
}

int tb_es_floats(int env_kind) {
  return env_kind == TB_ENV_SWING ? es_floats<TB_ENV_SWING>() : env_kind == TB_ENV_TENNIS ? es_floats<TB_ENV_TENNIS>() : TB_E_INVAL;
}

int tb_es_evaluate(TbHandle* h, const float* weights_dev, int n_members, size_t weights_stride_floats, int envs_per_member, double* return_dev,
                   int32_t* length_dev, const TbEsTrace* trace, void* stream) {
  if (!h || !weights_dev || !return_dev || !length_dev) return fail(TB_E_INVAL, "tb_es_evaluate: null argument");
  if (int rc = members_refused("tb_es_evaluate", h, n_members, envs_per_member, 1, weights_stride_floats, tb_es_floats(h->kind), weights_dev)) return rc;
  EsArgs E;
  memset(&E, 0, sizeof E);
  E.weights = weights_dev; E.stride = weights_stride_floats; E.per_member = envs_per_member; E.ret = return_dev; E.len = length_dev;
  if (trace && trace->max_steps > 0) {
    if (trace->struct_size < sizeof(TbEsTrace)) return fail(TB_E_INVAL, "tb_es_evaluate: TbEsTrace.struct_size too small");
    if (!trace->net_in || !trace->obs || !trace->actions || !trace->raw || !trace->reward || !trace->done)
      return fail(TB_E_INVAL, "tb_es_evaluate: a TbEsTrace array is null");
    E.t_max = trace->max_steps; E.t_net_in = trace->net_in; E.t_obs = trace->obs; E.t_act = trace->actions; E.t_raw = trace->raw;
    E.t_rew = trace->reward; E.t_done = trace->done;
  }
  return run_whole_episodes(h, "tb_es_evaluate", nullptr, return_dev, E.t_max, E.t_rew, stream, [&](const KArgs& a, bool rg, hipStream_t s) {
    const auto kern = kernel_of_kind_rg(h->kind, rg, [](auto K, auto R) { return tb_es_rollout_kernel<K.value, R.value>; });
    return launch(kern, dim3((unsigned)((h->n + 63) / 64)), dim3(64), dyn_lds(es_lds_words(h->kind, rg), 64), s, a, E);
  });
}

namespace {
// tb_policy_evaluate and tb_policy_evaluate_members (`who`; members: null, or the population whose blobs weights_dev holds: a
// workgroup's 16 envs belong to one member, and the kernel's members form runs on the same grid, block and LDS)
int policy_evaluate(const char* who, TbHandle* h, int net, const float* weights_dev, const PolicyMembers* members, int n_members, double* return_dev,
                    int32_t* length_dev, uint64_t noise_seed, int deterministic, void* stream) {
  if (!h || !weights_dev || !return_dev || !length_dev) return refusal(TB_E_INVAL, who, ": null argument");
  if (int rc = policy_net_ok(h->kind, net, who)) return rc;
  if (members) {
    if (int rc = members_refused(who, h, n_members, members->per_member, TB_POLICY_SLICE, members->stride, tb_policy_blob_floats(h->kind, net), weights_dev)) return rc;
  }
  PolicyIO pol = {};
  pol.weights = weights_dev; pol.seed = noise_seed; pol.deterministic = deterministic; pol.net = net;
  return run_whole_episodes(h, who, &pol, return_dev, 0, nullptr, stream, [&](const KArgs& a, bool rg, hipStream_t s) {
    const size_t lds = dyn_lds(policy_rollout_lds_words(h->kind, rg), 64);
    if (members) {
      const auto kern = kernel_of_kind_net_rg(h->kind, net, rg, [](auto K, auto N, auto R) { return tb_policy_evaluate_kernel<K.value, R.value, N.value, PolicyMembers>; });
      if (!kern) return fail(TB_E_UNSUPPORTED, "no tb_policy_evaluate_kernel members instantiation for this variant");
      return launch(kern, slice_groups(h), dim3(128), lds, s, a, return_dev, length_dev, *members);
    }
    const auto kern = kernel_of_kind_net_rg(h->kind, net, rg, [](auto K, auto N, auto R) { return tb_policy_evaluate_kernel<K.value, R.value, N.value>; });
    if (!kern) return fail(TB_E_UNSUPPORTED, "no tb_policy_evaluate_kernel instantiation for this variant");
    return launch(kern, slice_groups(h), dim3(128), lds, s, a, return_dev, length_dev);
  });
}
}  // namespace
int tb_policy_evaluate(TbHandle* h, int net, const float* weights_dev, double* return_dev, int32_t* length_dev, uint64_t noise_seed, int deterministic,
                       void* stream) {
  return policy_evaluate("tb_policy_evaluate", h, net, weights_dev, nullptr, 0, return_dev, length_dev, noise_seed, deterministic, stream);
}
int tb_policy_member_granule(void) { return TB_POLICY_SLICE; }
int tb_policy_evaluate_members(TbHandle* h, int net, const float* weights_dev, int n_members, size_t weights_stride_floats, int envs_per_member,
                               double* return_dev, int32_t* length_dev, uint64_t noise_seed, int deterministic, void* stream) {
  const PolicyMembers members = {weights_stride_floats, envs_per_member};
  return policy_evaluate("tb_policy_evaluate_members", h, net, weights_dev, &members, n_members, return_dev, length_dev, noise_seed, deterministic, stream);
}

// SAC's / TQC's actor inside the episode loop (tb_sac.hpp, tb_sac_evaluate_kernel), four waves per 16 envs: tb_sac_evaluate and
// tb_sac_evaluate_members (`who`; members: null, or the population of actors, as in policy_evaluate). The optional trace is checked last
namespace {
int sac_evaluate(const char* who, TbHandle* h, const float* actor_dev, const PolicyMembers* members, int n_members, double* return_dev, int32_t* length_dev,
                 uint64_t noise_seed, int deterministic, const TbSacEvalTrace* trace, void* stream) {
  if (!h || !actor_dev || !return_dev || !length_dev) return refusal(TB_E_INVAL, who, ": null argument");
  if (members) {
    if (int rc = members_refused(who, h, n_members, members->per_member, TB_POLICY_SLICE, members->stride, tb_sac_param_floats(h->kind, TB_SAC_ACTOR), actor_dev)) return rc;
  }
  SacEvalArgs S;
  memset(&S, 0, sizeof S);
  S.actor = actor_dev; S.ret = return_dev; S.len = length_dev;
  if (trace) {
    if (trace->struct_size != sizeof(TbSacEvalTrace)) return refusal(TB_E_INVAL, who, ": TbSacEvalTrace.struct_size is not sizeof(TbSacEvalTrace)");
    if (trace->max_steps > 0) {
      if (!trace->obs || !trace->eps || !trace->actions || !trace->reward || !trace->done) return refusal(TB_E_INVAL, who, ": a TbSacEvalTrace array is null");
      S.t_max = trace->max_steps; S.t_obs = trace->obs; S.t_eps = trace->eps; S.t_act = trace->actions; S.t_rew = trace->reward; S.t_done = trace->done;
    }
  }
  PolicyIO pol = {};
  pol.seed = noise_seed; pol.deterministic = deterministic;
  return run_whole_episodes(h, who, &pol, return_dev, S.t_max, S.t_rew, stream, [&](const KArgs& a, bool rg, hipStream_t s) {
    const size_t lds = dyn_lds(policy_rollout_lds_words(h->kind, rg), 64);
    if (members)
      return launch(kernel_of_kind_rg(h->kind, rg, [](auto K, auto R) { return tb_sac_evaluate_kernel<K.value, R.value, PolicyMembers>; }), slice_groups(h), dim3(256), lds, s, a,
                    S, *members);
    return launch(kernel_of_kind_rg(h->kind, rg, [](auto K, auto R) { return tb_sac_evaluate_kernel<K.value, R.value>; }), slice_groups(h), dim3(256), lds, s, a, S);
  });
}
}  // namespace
int tb_sac_evaluate(TbHandle* h, const float* actor_dev, double* return_dev, int32_t* length_dev, uint64_t noise_seed, int deterministic,
                    const TbSacEvalTrace* trace, void* stream) {
  return sac_evaluate("tb_sac_evaluate", h, actor_dev, nullptr, 0, return_dev, length_dev, noise_seed, deterministic, trace, stream);
}
int tb_sac_evaluate_members(TbHandle* h, const float* actors_dev, int n_members, size_t actors_stride_floats, int envs_per_member, double* return_dev,
                            int32_t* length_dev, uint64_t noise_seed, int deterministic, const TbSacEvalTrace* trace, void* stream) {
  const PolicyMembers members = {actors_stride_floats, envs_per_member};
  return sac_evaluate("tb_sac_evaluate_members", h, actors_dev, &members, n_members, return_dev, length_dev, noise_seed, deterministic, trace, stream);
}

// tb_sac_collect_kernel (tb_sac.hpp): one launch, the caller's ring rows as outputs
int tb_sac_collect(TbHandle* h, const float* actor_dev, int n_steps, int mode, uint64_t noise_seed, const TbSacCollectOut* out, void* stream) {
  if (!h || !out) return fail(TB_E_INVAL, "tb_sac_collect: null argument");
  if (out->struct_size != sizeof(TbSacCollectOut)) return fail(TB_E_INVAL, "tb_sac_collect: TbSacCollectOut.struct_size is not sizeof(TbSacCollectOut)");
  if (!out->obs || !out->next_obs || !out->action || !out->reward || !out->done) return fail(TB_E_INVAL, "tb_sac_collect: a TbSacCollectOut array is null");
  if (mode != TB_SAC_COLLECT_ACTOR && mode != TB_SAC_COLLECT_UNIFORM) return fail(TB_E_INVAL, "tb_sac_collect: unknown mode");
  if (mode == TB_SAC_COLLECT_ACTOR && !actor_dev) return fail(TB_E_INVAL, "tb_sac_collect: actor_dev is null in actor mode");
  if (n_steps < 1) return fail(TB_E_INVAL, "tb_sac_collect: n_steps must be >= 1");
  if (int rc = refuse_steps_from_state(h, "tb_sac_collect")) return rc;
  const bool swing = h->kind == TB_ENV_SWING;
  if (swing && h->phase.at + n_steps > kEpisodeSteps)
    return fail(TB_E_INVAL, "tb_sac_collect on SwingRacket-v0: the launch must end where the episodes do at the latest (phase + n_steps <= 26)");
  const uintptr_t row_align = swing ? 8 : 16;  // write_obs: float2 / float4 stores
  if ((reinterpret_cast<uintptr_t>(out->obs) | reinterpret_cast<uintptr_t>(out->next_obs)) % row_align ||
      (reinterpret_cast<uintptr_t>(out->action) | reinterpret_cast<uintptr_t>(out->eps_or_null)) % 8 ||
      (reinterpret_cast<uintptr_t>(out->reward) | reinterpret_cast<uintptr_t>(out->done)) % sizeof(float))
    return fail(TB_E_INVAL, "tb_sac_collect: obs / next_obs must be 16-byte aligned (SwingRacket-v0: 8), action / eps 8-byte, reward / done 4-byte");
  DeviceGuard g(h->device);
  hipStream_t s = (hipStream_t)stream;
  SacCollectArgs S;
  memset(&S, 0, sizeof S);
  S.actor = actor_dev; S.n_steps = n_steps; S.uniform = mode == TB_SAC_COLLECT_UNIFORM;
  S.obs = out->obs; S.next_obs = out->next_obs; S.action = out->action; S.reward = out->reward; S.done = out->done; S.eps = out->eps_or_null;
  KArgs a = base_args(h);
  a.pol_seed = noise_seed; a.pol_deterministic = 0;
  a.reward = out->reward; a.T = n_steps;  // (SwingRacket: the fast-forward's destination is the row of the launch's last step)
  return run_steps_from_state(h, n_steps, a, (size_t)h->n, true, s, [&](const KArgs& k, bool rg) {
    const auto kern = kernel_of_kind_rg(h->kind, rg, [](auto K, auto R) { return tb_sac_collect_kernel<K.value, R.value>; });
    return launch(kern, slice_groups(h), dim3(256), dyn_lds(policy_rollout_lds_words(h->kind, rg), 64), s, k, S);
  });
}

// ------------------------------------------------------------------------------------------ the PPO learner (tb_learner.hpp)
int tb_ppo_param_floats(int env_kind) {
  return env_kind == TB_ENV_SWING ? PpoLayout<TB_ENV_SWING>::P : env_kind == TB_ENV_TENNIS ? PpoLayout<TB_ENV_TENNIS>::P : TB_E_INVAL;
}
extern "C++" {
namespace {
// PpoLayout<KIND, NET> / TunedLayout at run time: the flat vector's length, the floats of one partial vector (the gradient and the two
// statistics; the tuned net's also hold the vf waves' extractor share) and where the value slots lie -- zeros for the tuned net, whose
// extractor is shared: it has no critic-only range. THE place that maps a (kind, net) pair to a layout; any other pair gives zeros.
struct PpoDims { int P, STRIDE, VF, PI_HEAD, VF_HEAD; };
PpoDims ppo_dims(int env_kind, int net) {
  return with_kind_net(env_kind, net, PpoDims{}, [](auto K, auto N) -> PpoDims {
    if constexpr (N.value == TB_NET_TUNED) return {TunedLayout::P, TunedLayout::STRIDE, 0, 0, 0};
    else {
      using L = PpoLayout<K.value, N.value>;
      return {L::P, L::P + 2, L::VF, L::PI_HEAD, L::VF_HEAD};
    }
  });
}
size_t ppo_partials(int batch) { return 2 * (((size_t)batch + TB_PPO_SHARE - 1) / TB_PPO_SHARE); }
constexpr size_t kPpoStatBytes = sizeof(double) * 2 * TB_PPO_STAT_BLOCKS;
bool misaligned(const void* p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a != 0; }

// The learner calls name their device by index, and look it up only once every argument has passed: `who`'s refusal if there is no
// device or no such index, else g makes it current for the rest of the call.
int learner_device(DeviceGuard& g, int device, const char* who) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(TB_E_NODEVICE, "tb_ppo: no HIP device available (this library has no CPU fallback)");
  if (device < 0 || device >= ndev) return refusal(TB_E_NODEVICE, who, ": device index out of range");
  g.enter(device);
  return g.err == hipSuccess ? TB_OK : fail((int)g.err, "hipSetDevice");
}
// A rollout's rewards and dones, rows one step apart: their step strides in elements from the caller's in bytes (0: packed, n_envs)
int step_strides(const char* who, int n_envs, size_t reward_bytes, size_t done_bytes, size_t* rs, size_t* ds) {
  *rs = *ds = (size_t)n_envs;
  if (reward_bytes) {
    if (reward_bytes % sizeof(float) || reward_bytes < sizeof(float) * (size_t)n_envs)
      return refusal(TB_E_INVAL, who, ": the rewards' step stride must be a multiple of 4 bytes and hold n_envs floats");
    *rs = reward_bytes / sizeof(float);
  }
  if (done_bytes) {
    if (done_bytes < (size_t)n_envs) return refusal(TB_E_INVAL, who, ": the dones' step stride is shorter than n_envs bytes");
    *ds = done_bytes;
  }
  return TB_OK;
}
}  // namespace
}  // extern "C++"
int tb_ppo_param_floats_net(int env_kind, int net) {
  if (!kind_ok(env_kind)) return TB_E_INVAL;
  if (int rc = policy_net_ok(env_kind, net, "tb_ppo_param_floats_net")) return rc;
  return ppo_dims(env_kind, net).P;
}
int tb_ppo_rows_per_workgroup(void) { return TB_PPO_SHARE; }

long long tb_ppo_workspace_bytes_net(int env_kind, int net, int batch) {
  if (!kind_ok(env_kind) || batch < 2) return fail(TB_E_INVAL, "tb_ppo_workspace_bytes: unknown env kind, or batch < 2");
  if (int rc = policy_net_ok(env_kind, net, "tb_ppo_workspace_bytes_net")) return rc;
  return (long long)(kPpoStatBytes + sizeof(float) * ppo_partials(batch) * (size_t)ppo_dims(env_kind, net).STRIDE);
}
long long tb_ppo_workspace_bytes(int env_kind, int batch) { return tb_ppo_workspace_bytes_net(env_kind, TB_NET_DEFAULT, batch); }
// a population's workspace: one learner's per member, a multiple of 8 bytes apart
long long tb_ppo_members_workspace_stride_bytes(int env_kind, int net, int batch) {
  const long long one = tb_ppo_workspace_bytes_net(env_kind, net, batch);
  return one < 0 ? one : (one + 7) / 8 * 8;
}

int tb_ppo_gae(int env_kind, int device, void* stream, int n_steps, int n_envs, const float* rewards_dev, size_t reward_step_stride_bytes,
               const uint8_t* dones_dev, size_t done_step_stride_bytes, const float* values_dev, const float* last_value_dev, double gamma,
               double gae_lambda, float* adv_dev, float* returns_dev) {
  if (!kind_ok(env_kind)) return fail(TB_E_INVAL, "tb_ppo_gae: unknown env kind");
  if (!rewards_dev || !dones_dev || !values_dev || !last_value_dev || !adv_dev || !returns_dev) return fail(TB_E_INVAL, "tb_ppo_gae: null argument");
  if (n_steps < 1 || n_envs < 1) return fail(TB_E_INVAL, "tb_ppo_gae: n_steps and n_envs must be >= 1");
  if (misaligned(rewards_dev, 4) || misaligned(values_dev, 4) || misaligned(last_value_dev, 4) || misaligned(adv_dev, 4) || misaligned(returns_dev, 4))
    return fail(TB_E_INVAL, "tb_ppo_gae: a float array is not 4-byte aligned");
  size_t rs, ds;
  if (int rc = step_strides("tb_ppo_gae", n_envs, reward_step_stride_bytes, done_step_stride_bytes, &rs, &ds)) return rc;
  DeviceGuard g;
  if (int rc = learner_device(g, device, "tb_ppo_gae")) return rc;
  return launch(tb_ppo_gae_kernel, dim3((unsigned)((n_envs + 63) / 64)), dim3(64), 0, (hipStream_t)stream, n_steps, n_envs, rewards_dev, rs, dones_dev, ds,
                values_dev, last_value_dev, (float)gamma, (float)(gamma * gae_lambda), adv_dev, returns_dev);
}

// ---- a minibatch step, for one learner and for a population (tb_learner.hpp, "THE MEMBER AXIS": the same kernels with the member as a
// second grid axis). Each stage is written once: mb is nothing, or the population's PpoMembers, which the kernels take the same way.
extern "C++" {
namespace {
const PpoMembers* population() { return nullptr; }
const PpoMembers* population(const PpoMembers& mb) { return &mb; }

// What both stages refuse before the device is looked up (pop: null for one learner). First the pair: the kind, then the net
// (TB_E_PARAMS). arrays_null: a population's null array is TB_E_INVAL whatever the pair; one learner's is, under a pair that is built ...
int ppo_pair_refused(const char* who, int env_kind, int net, bool arrays_null) {
  if (arrays_null) return refusal(TB_E_INVAL, who, ": null argument");
  if (!kind_ok(env_kind)) return refusal(TB_E_INVAL, who, ": unknown env kind");
  return policy_net_ok(env_kind, net, who);
}
// ... then the buffers. any_null, float_off, idx_off: over the stage's own arrays (null; not 4-byte aligned; idx not 8-byte aligned).
// with_workspace: the call reads or writes the workspace (all but tb_ppo_apply without TB_PPO_REDUCE), so it and the batch are checked.
int ppo_buffers_refused(const char* who, int env_kind, int net, int n_params, bool any_null, bool float_off, bool idx_off, bool with_workspace, int batch,
                        const void* workspace_dev, size_t workspace_bytes, const PpoMembers* pop, int n_members) {
  if (pop && (n_members < 1 || n_members > 65535)) return refusal(TB_E_INVAL, who, ": n_members must be in [1, 65535] (the member is a grid axis)");
  if (with_workspace && batch < 2) return refusal(TB_E_INVAL, who, ": batch must be >= 2 (the unbiased std of one row is undefined)");
  if (any_null || (with_workspace && !workspace_dev) || (pop && !pop->hp)) return refusal(TB_E_INVAL, who, ": null argument");
  if (n_params != tb_ppo_param_floats_net(env_kind, net)) return refusal(TB_E_INVAL, who, ": n_params is not tb_ppo_param_floats_net(env_kind, net)");
  if (pop && pop->param_stride < (size_t)n_params) return refusal(TB_E_INVAL, who, ": param_stride_floats is shorter than n_params");
  if (float_off) return refusal(TB_E_INVAL, who, ": a float array is not 4-byte aligned");
  if (idx_off || (with_workspace && misaligned(workspace_dev, 8)) || (pop && misaligned(pop->hp, 8)))
    return refusal(TB_E_INVAL, who, ": idx, hp and the workspace must be 8-byte aligned");
  if (with_workspace && workspace_bytes / (size_t)(pop ? n_members : 1) < (pop ? pop->ws_stride : (size_t)tb_ppo_workspace_bytes_net(env_kind, net, batch)))
    return refusal(TB_E_INVAL, who, ": the workspace is smaller than tb_ppo_workspace_bytes (a population's: n_members * tb_ppo_members_workspace_stride_bytes)");
  return TB_OK;
}

// tb_ppo_grad_net and tb_ppo_grad_members (`who`). n_members: the grid's second axis, 1 for one learner; a population's clip_range and
// vf_coef are each member's own, from hp
template <class... MB>
int ppo_grad(const char* who, int env_kind, int net, int device, void* stream, const float* obs_dev, const float* raw_actions_dev, const float* old_logp_dev,
             const float* adv_dev, const float* returns_dev, long long n_rows, const int64_t* idx_dev, int batch, int n_members, const float* params_dev, int n_params,
             float clip_range, float vf_coef, void* workspace_dev, size_t workspace_bytes, const MB&... mb) {
  const PpoMembers* const pop = population(mb...);
  const bool any_null = !obs_dev || !raw_actions_dev || !old_logp_dev || !adv_dev || !returns_dev || !idx_dev || !params_dev;
  if (int rc = ppo_pair_refused(who, env_kind, net, pop && any_null)) return rc;
  if (int rc = ppo_buffers_refused(who, env_kind, net, n_params, any_null,
                                   misaligned(obs_dev, 4) || misaligned(raw_actions_dev, 4) || misaligned(old_logp_dev, 4) || misaligned(adv_dev, 4) ||
                                       misaligned(returns_dev, 4) || misaligned(params_dev, 4),
                                   misaligned(idx_dev, 8), true, batch, workspace_dev, workspace_bytes, pop, n_members))
    return rc;
  if (n_rows < 1) return refusal(TB_E_INVAL, who, ": n_rows must be >= 1");
  if (pop && pop->idx_stride < (size_t)batch) return refusal(TB_E_INVAL, who, ": idx_stride is shorter than batch");
  DeviceGuard g;
  if (int rc = learner_device(g, device, who)) return rc;
  hipStream_t s = (hipStream_t)stream;
  double* sums = (double*)workspace_dev;
  const PpoGradArgs a = {obs_dev, raw_actions_dev, old_logp_dev, adv_dev, returns_dev, (const long long*)idx_dev, params_dev, sums,
                         (float*)((char*)workspace_dev + kPpoStatBytes), n_rows, batch, clip_range, vf_coef};
  const unsigned M = (unsigned)n_members;
  if (int rc = launch(tb_ppo_adv_stats_kernel<MB...>, dim3(TB_PPO_STAT_BLOCKS, M), dim3(256), 0, s, adv_dev, (const long long*)idx_dev, batch, n_rows, sums, mb...)) return rc;
  const dim3 grid((unsigned)(ppo_partials(batch) / 2), M);
  return with_kind_net(env_kind, net, TB_E_UNSUPPORTED, [&](auto K, auto N) {
    if constexpr (N.value == TB_NET_TUNED) return launch(tb_ppo_grad_tuned_kernel<MB...>, grid, dim3(256), 0, s, a, mb...);
    else return launch(tb_ppo_grad_kernel<K.value, N.value, MB...>, grid, dim3(256), 0, s, a, mb...);
  });
}

// tb_ppo_apply_net and tb_ppo_apply_members (`who`): the reduce and the Adam step. A population runs both phases, never value-only, with
// world = 1; its ent_coef and lr are each member's own, from hp
template <class... MB>
int ppo_apply(const char* who, int env_kind, int net, int device, void* stream, int phases, const void* workspace_dev, size_t workspace_bytes, int batch, int n_members,
              float* params_dev, float* grad_dev, float* exp_avg_dev, float* exp_avg_sq_dev, int n_params, float* stats_dev, float ent_coef, float max_grad_norm,
              int world, float lr, float beta1, float beta2, float eps, long long step, const MB&... mb) {
  const PpoMembers* const pop = population(mb...);
  const bool reduce = (phases & TB_PPO_REDUCE) != 0, adam = (phases & TB_PPO_STEP) != 0;
  const int value_only = (phases & TB_PPO_VALUE_ONLY) != 0;
  const bool any_null = !params_dev || !grad_dev || (reduce && !stats_dev) || (adam && (!exp_avg_dev || !exp_avg_sq_dev));
  if (int rc = ppo_pair_refused(who, env_kind, net, pop && any_null)) return rc;
  if (net == TB_NET_TUNED && value_only)
    return refusal(TB_E_UNSUPPORTED, who, ": TB_PPO_VALUE_ONLY is not offered for TB_NET_TUNED (the extractor is shared: there is no critic-only slot range)");
  if (!(reduce || adam) || (phases & ~(TB_PPO_REDUCE | TB_PPO_STEP | TB_PPO_VALUE_ONLY)))
    return refusal(TB_E_INVAL, who, ": phases must be TB_PPO_REDUCE, TB_PPO_STEP or both, with or without TB_PPO_VALUE_ONLY");
  if (int rc = ppo_buffers_refused(who, env_kind, net, n_params, any_null,
                                   misaligned(params_dev, 4) || misaligned(grad_dev, 4) || misaligned(exp_avg_dev, 4) || misaligned(exp_avg_sq_dev, 4) ||
                                       misaligned(stats_dev, 4),
                                   false, reduce, batch, workspace_dev, workspace_bytes, pop, n_members))
    return rc;
  if (adam && (world < 1 || step < 1)) return refusal(TB_E_INVAL, who, ": world and step must be >= 1");
  DeviceGuard g;
  if (int rc = learner_device(g, device, who)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const unsigned M = (unsigned)n_members;
  if (reduce) {
    const float* partials = (const float*)((const char*)workspace_dev + kPpoStatBytes);
    const float* params = params_dev;
    const int n_part = (int)ppo_partials(batch);
    const dim3 grid((unsigned)((n_params + 2 + 63) / 64), M);
    // (the tuned net's reduce is its own kernel, without a value-only form)
    if (int rc = with_kind_net(env_kind, net, TB_E_UNSUPPORTED, [&](auto K, auto N) {
          if constexpr (N.value == TB_NET_TUNED) return launch(tb_ppo_reduce_tuned_kernel<MB...>, grid, dim3(256), 0, s, partials, n_part, batch, params, ent_coef, grad_dev, stats_dev, mb...);
          else return launch(tb_ppo_reduce_kernel<K.value, N.value, MB...>, grid, dim3(256), 0, s, partials, n_part, batch, params, ent_coef, grad_dev, stats_dev, value_only, mb...);
        }))
      return rc;
  }
  if (adam) {
    const float c1 = (float)(1.0 - pow((double)beta1, (double)step)), c2 = (float)(1.0 - pow((double)beta2, (double)step));
    int lo0 = 0, hi0 = n_params, lo1 = 0, hi1 = 0;
    if (value_only) {  // the critic's slots alone
      const PpoDims d = ppo_dims(env_kind, net);
      lo0 = d.VF; hi0 = d.PI_HEAD; lo1 = d.VF_HEAD; hi1 = d.P;
    }
    return launch(tb_ppo_step_kernel<MB...>, dim3(M), dim3(1024), 0, s, params_dev, grad_dev, exp_avg_dev, exp_avg_sq_dev, n_params, (float)world, max_grad_norm, lr,
                  beta1, beta2, eps, c1, c2, lo0, hi0, lo1, hi1, mb...);
  }
  return TB_OK;
}
}  // namespace
}  // extern "C++"

int tb_ppo_grad(int env_kind, int device, void* stream, const float* obs_dev, const float* raw_actions_dev, const float* old_logp_dev, const float* adv_dev,
                const float* returns_dev, long long n_rows, const int64_t* idx_dev, int batch, const float* params_dev, int n_params, float clip_range,
                float vf_coef, void* workspace_dev, size_t workspace_bytes) {
  return tb_ppo_grad_net(env_kind, TB_NET_DEFAULT, device, stream, obs_dev, raw_actions_dev, old_logp_dev, adv_dev, returns_dev, n_rows, idx_dev, batch, params_dev,
                         n_params, clip_range, vf_coef, workspace_dev, workspace_bytes);
}
int tb_ppo_grad_net(int env_kind, int net, int device, void* stream, const float* obs_dev, const float* raw_actions_dev, const float* old_logp_dev,
                    const float* adv_dev, const float* returns_dev, long long n_rows, const int64_t* idx_dev, int batch, const float* params_dev, int n_params,
                    float clip_range, float vf_coef, void* workspace_dev, size_t workspace_bytes) {
  return ppo_grad("tb_ppo_grad", env_kind, net, device, stream, obs_dev, raw_actions_dev, old_logp_dev, adv_dev, returns_dev, n_rows, idx_dev, batch, 1, params_dev,
                  n_params, clip_range, vf_coef, workspace_dev, workspace_bytes);
}
int tb_ppo_grad_members(int env_kind, int net, int device, void* stream, const float* obs_dev, const float* raw_actions_dev, const float* old_logp_dev,
                        const float* adv_dev, const float* returns_dev, long long n_rows, const int64_t* idx_dev, size_t idx_stride, int batch, int n_members,
                        const float* params_dev, size_t param_stride_floats, int n_params, const TbPpoMemberHp* hp_dev, void* workspace_dev, size_t workspace_bytes) {
  const PpoMembers mb = {hp_dev, idx_stride, param_stride_floats, (size_t)tb_ppo_members_workspace_stride_bytes(env_kind, net, batch)};
  return ppo_grad("tb_ppo_grad_members", env_kind, net, device, stream, obs_dev, raw_actions_dev, old_logp_dev, adv_dev, returns_dev, n_rows, idx_dev, batch, n_members,
                  params_dev, n_params, 0.0f, 0.0f, workspace_dev, workspace_bytes, mb);
}

int tb_ppo_apply(int env_kind, int device, void* stream, int phases, const void* workspace_dev, size_t workspace_bytes, int batch, float* params_dev,
                 float* grad_dev, float* exp_avg_dev, float* exp_avg_sq_dev, int n_params, float* stats_dev, float ent_coef, float max_grad_norm, int world,
                 float lr, float beta1, float beta2, float eps, long long step) {
  return tb_ppo_apply_net(env_kind, TB_NET_DEFAULT, device, stream, phases, workspace_dev, workspace_bytes, batch, params_dev, grad_dev, exp_avg_dev, exp_avg_sq_dev,
                          n_params, stats_dev, ent_coef, max_grad_norm, world, lr, beta1, beta2, eps, step);
}
int tb_ppo_apply_net(int env_kind, int net, int device, void* stream, int phases, const void* workspace_dev, size_t workspace_bytes, int batch, float* params_dev,
                     float* grad_dev, float* exp_avg_dev, float* exp_avg_sq_dev, int n_params, float* stats_dev, float ent_coef, float max_grad_norm, int world,
                     float lr, float beta1, float beta2, float eps, long long step) {
  return ppo_apply("tb_ppo_apply", env_kind, net, device, stream, phases, workspace_dev, workspace_bytes, batch, 1, params_dev, grad_dev, exp_avg_dev, exp_avg_sq_dev,
                   n_params, stats_dev, ent_coef, max_grad_norm, world, lr, beta1, beta2, eps, step);
}
int tb_ppo_apply_members(int env_kind, int net, int device, void* stream, const void* workspace_dev, size_t workspace_bytes, int batch, int n_members,
                         float* params_dev, float* grad_dev, float* exp_avg_dev, float* exp_avg_sq_dev, size_t param_stride_floats, int n_params, float* stats_dev,
                         const TbPpoMemberHp* hp_dev, float max_grad_norm, float beta1, float beta2, float eps, long long step) {
  const PpoMembers mb = {hp_dev, 0, param_stride_floats, (size_t)tb_ppo_members_workspace_stride_bytes(env_kind, net, batch)};
  return ppo_apply("tb_ppo_apply_members", env_kind, net, device, stream, TB_PPO_REDUCE | TB_PPO_STEP, workspace_dev, workspace_bytes, batch, n_members, params_dev, grad_dev,
                   exp_avg_dev, exp_avg_sq_dev, n_params, stats_dev, 0.0f, max_grad_norm, 1, 0.0f, beta1, beta2, eps, step, mb);
}

// ------------------------------------------------------------------------------------------- the TRPO learner (tb_trpo.hpp)
int tb_trpo_rows_per_workgroup(void) { return TB_PPO_SHARE; }
int tb_trpo_search_rows_per_workgroup(void) { return TB_TRPO_SEARCH_SHARE; }

static size_t trpo_search_shares(int batch) { return ((size_t)batch + TB_TRPO_SEARCH_SHARE - 1) / TB_TRPO_SEARCH_SHARE; }
// the pairs the TRPO kernels are built for: with_kind_net's without the tuned network (trpo_net_ok has refused it by then)
extern "C++" {
template <class F>
static int with_trpo_kind_net(int kind, int net, F f) {
  return with_kind_net(kind, net, TB_E_UNSUPPORTED, [&](auto K, auto N) {
    if constexpr (N.value == TB_NET_TUNED) return TB_E_UNSUPPORTED;
    else return f(K, N);
  });
}
}

long long tb_trpo_fvp_workspace_bytes_net(int env_kind, int net, int n_idx) {
  if (!kind_ok(env_kind) || n_idx < 1) return fail(TB_E_INVAL, "tb_trpo_fvp_workspace_bytes: unknown env kind, or n_idx < 1");
  if (int rc = trpo_net_ok(env_kind, net, "tb_trpo_fvp_workspace_bytes_net")) return rc;
  return (long long)(sizeof(float) * ppo_partials(n_idx) * (size_t)tb_ppo_param_floats_net(env_kind, net));
}
long long tb_trpo_fvp_workspace_bytes(int env_kind, int n_idx) { return tb_trpo_fvp_workspace_bytes_net(env_kind, TB_NET_DEFAULT, n_idx); }
long long tb_trpo_search_workspace_bytes_net(int env_kind, int net, int batch, int n_candidates) {
  if (!kind_ok(env_kind) || batch < 2 || n_candidates < 1 || n_candidates > TB_TRPO_MAX_CANDIDATES)
    return fail(TB_E_INVAL, "tb_trpo_search_workspace_bytes: unknown env kind, batch < 2, or n_candidates outside 1 .. 64");
  if (int rc = trpo_net_ok(env_kind, net, "tb_trpo_search_workspace_bytes_net")) return rc;
  return (long long)(kPpoStatBytes + sizeof(double) * 2 * trpo_search_shares(batch) * (size_t)n_candidates);
}
long long tb_trpo_search_workspace_bytes(int env_kind, int batch, int n_candidates) {
  return tb_trpo_search_workspace_bytes_net(env_kind, TB_NET_DEFAULT, batch, n_candidates);
}

int tb_trpo_fvp(int env_kind, int device, void* stream, const float* obs_dev, long long n_rows, const int64_t* idx_dev, int n_idx, const float* params_dev,
                const float* vec_dev, int n_params, float damping, float* out_dev, void* workspace_dev, size_t workspace_bytes) {
  return tb_trpo_fvp_net(env_kind, TB_NET_DEFAULT, device, stream, obs_dev, n_rows, idx_dev, n_idx, params_dev, vec_dev, n_params, damping, out_dev, workspace_dev,
                         workspace_bytes);
}
int tb_trpo_fvp_net(int env_kind, int net, int device, void* stream, const float* obs_dev, long long n_rows, const int64_t* idx_dev, int n_idx,
                    const float* params_dev, const float* vec_dev, int n_params, float damping, float* out_dev, void* workspace_dev, size_t workspace_bytes) {
  if (!kind_ok(env_kind)) return fail(TB_E_INVAL, "tb_trpo_fvp: unknown env kind");
  if (int rc = trpo_net_ok(env_kind, net, "tb_trpo_fvp")) return rc;
  if (!obs_dev || !idx_dev || !params_dev || !vec_dev || !out_dev || !workspace_dev) return fail(TB_E_INVAL, "tb_trpo_fvp: null argument");
  if (n_params != tb_ppo_param_floats_net(env_kind, net)) return fail(TB_E_INVAL, "tb_trpo_fvp: n_params is not tb_ppo_param_floats_net(env_kind, net)");
  if (n_rows < 1 || n_idx < 1) return fail(TB_E_INVAL, "tb_trpo_fvp: n_rows and n_idx must be >= 1");
  if (misaligned(obs_dev, 4) || misaligned(params_dev, 4) || misaligned(vec_dev, 4) || misaligned(out_dev, 4))
    return fail(TB_E_INVAL, "tb_trpo_fvp: a float array is not 4-byte aligned");
  if (misaligned(idx_dev, 8) || misaligned(workspace_dev, 8)) return fail(TB_E_INVAL, "tb_trpo_fvp: idx and the workspace must be 8-byte aligned");
  if (vec_dev == out_dev) return fail(TB_E_INVAL, "tb_trpo_fvp: out_dev must not be vec_dev");
  if ((long long)workspace_bytes < tb_trpo_fvp_workspace_bytes_net(env_kind, net, n_idx)) return fail(TB_E_INVAL, "tb_trpo_fvp: the workspace is smaller than tb_trpo_fvp_workspace_bytes");
  DeviceGuard g;
  if (int rc = learner_device(g, device, "tb_trpo_fvp")) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int n_part = (int)ppo_partials(n_idx);
  TrpoFvpArgs a = {obs_dev, (const long long*)idx_dev, params_dev, vec_dev, (float*)workspace_dev, n_rows, n_idx};
  const dim3 grid((unsigned)(n_part / 2)), rgrid((unsigned)((n_params + 63) / 64));
  return with_trpo_kind_net(env_kind, net, [&](auto K, auto N) {
    if (int rc = launch(tb_trpo_fvp_kernel<K.value, N.value>, grid, dim3(128), 0, s, a)) return rc;
    return launch(tb_trpo_fvp_reduce_kernel<K.value, N.value>, rgrid, dim3(256), 0, s, (const float*)workspace_dev, n_part, n_idx, vec_dev, damping, out_dev);
  });
}

int tb_trpo_search(int env_kind, int device, void* stream, const float* obs_dev, const float* raw_actions_dev, const float* old_logp_dev, const float* adv_dev,
                   long long n_rows, const int64_t* idx_dev, int batch, const float* params_dev, const float* direction_dev, int n_params,
                   const float* steps_dev, int n_candidates, double* out_dev, void* workspace_dev, size_t workspace_bytes) {
  return tb_trpo_search_net(env_kind, TB_NET_DEFAULT, device, stream, obs_dev, raw_actions_dev, old_logp_dev, adv_dev, n_rows, idx_dev, batch, params_dev, direction_dev,
                            n_params, steps_dev, n_candidates, out_dev, workspace_dev, workspace_bytes);
}
int tb_trpo_search_net(int env_kind, int net, int device, void* stream, const float* obs_dev, const float* raw_actions_dev, const float* old_logp_dev,
                       const float* adv_dev, long long n_rows, const int64_t* idx_dev, int batch, const float* params_dev, const float* direction_dev, int n_params,
                       const float* steps_dev, int n_candidates, double* out_dev, void* workspace_dev, size_t workspace_bytes) {
  if (!kind_ok(env_kind)) return fail(TB_E_INVAL, "tb_trpo_search: unknown env kind");
  if (int rc = trpo_net_ok(env_kind, net, "tb_trpo_search")) return rc;
  if (!obs_dev || !raw_actions_dev || !old_logp_dev || !adv_dev || !idx_dev || !params_dev || !direction_dev || !steps_dev || !out_dev || !workspace_dev)
    return fail(TB_E_INVAL, "tb_trpo_search: null argument");
  if (n_params != tb_ppo_param_floats_net(env_kind, net)) return fail(TB_E_INVAL, "tb_trpo_search: n_params is not tb_ppo_param_floats_net(env_kind, net)");
  if (n_rows < 1 || batch < 2) return fail(TB_E_INVAL, "tb_trpo_search: n_rows must be >= 1 and batch >= 2 (the unbiased std of one row is undefined)");
  if (n_candidates < 1 || n_candidates > TB_TRPO_MAX_CANDIDATES) return fail(TB_E_INVAL, "tb_trpo_search: n_candidates must be 1 .. 64");
  if (misaligned(obs_dev, 4) || misaligned(raw_actions_dev, 4) || misaligned(old_logp_dev, 4) || misaligned(adv_dev, 4) || misaligned(params_dev, 4) ||
      misaligned(direction_dev, 4) || misaligned(steps_dev, 4))
    return fail(TB_E_INVAL, "tb_trpo_search: a float array is not 4-byte aligned");
  if (misaligned(idx_dev, 8) || misaligned(workspace_dev, 8) || misaligned(out_dev, 8))
    return fail(TB_E_INVAL, "tb_trpo_search: idx, out and the workspace must be 8-byte aligned");
  if ((long long)workspace_bytes < tb_trpo_search_workspace_bytes_net(env_kind, net, batch, n_candidates))
    return fail(TB_E_INVAL, "tb_trpo_search: the workspace is smaller than tb_trpo_search_workspace_bytes");
  DeviceGuard g;
  if (int rc = learner_device(g, device, "tb_trpo_search")) return rc;
  hipStream_t s = (hipStream_t)stream;
  double* sums = (double*)workspace_dev;
  double* partials = (double*)((char*)workspace_dev + kPpoStatBytes);
  const int shares = (int)trpo_search_shares(batch);
  TrpoSearchArgs a = {obs_dev, raw_actions_dev, old_logp_dev, adv_dev, (const long long*)idx_dev, params_dev, direction_dev, steps_dev, sums, partials, n_rows, batch};
  if (int rc = launch(tb_ppo_adv_stats_kernel<>, dim3(TB_PPO_STAT_BLOCKS), dim3(256), 0, s, adv_dev, (const long long*)idx_dev, batch, n_rows, sums)) return rc;
  const dim3 grid((unsigned)shares, (unsigned)n_candidates);
  if (int rc = with_trpo_kind_net(env_kind, net, [&](auto K, auto N) { return launch(tb_trpo_search_kernel<K.value, N.value>, grid, dim3(256), 0, s, a); })) return rc;
  return launch(tb_trpo_search_reduce_kernel, dim3((unsigned)n_candidates), dim3(256), 0, s, (const double*)partials, shares, batch, out_dev);
}

// the workspace of tb_trpo_returns: the [T][chunks] table of counts / offsets (int64), then L_e (int32 [n])
static long long trpo_return_chunks(int n_envs) { return ((long long)n_envs + 63) / 64; }
long long tb_trpo_returns_workspace_bytes(int n_steps, int n_envs) {
  if (n_steps < 1 || n_envs < 1) return fail(TB_E_INVAL, "tb_trpo_returns_workspace_bytes: n_steps and n_envs must be >= 1");
  return 8 * (long long)n_steps * trpo_return_chunks(n_envs) + 8 * (((long long)n_envs + 1) / 2);
}

int tb_trpo_returns(int env_kind, int device, void* stream, int n_steps, int n_envs, const float* rewards_dev, size_t reward_step_stride_bytes,
                    const uint8_t* dones_dev, size_t done_step_stride_bytes, double discount, float* returns_dev, int64_t* idx_dev, int64_t* count_dev,
                    void* workspace_dev, size_t workspace_bytes) {
  if (!kind_ok(env_kind)) return fail(TB_E_INVAL, "tb_trpo_returns: unknown env kind");
  if (!rewards_dev || !dones_dev || !returns_dev || !idx_dev || !count_dev || !workspace_dev) return fail(TB_E_INVAL, "tb_trpo_returns: null argument");
  if (n_steps < 1 || n_envs < 1) return fail(TB_E_INVAL, "tb_trpo_returns: n_steps and n_envs must be >= 1");
  if (misaligned(rewards_dev, 4) || misaligned(returns_dev, 4)) return fail(TB_E_INVAL, "tb_trpo_returns: a float array is not 4-byte aligned");
  if (misaligned(idx_dev, 8) || misaligned(count_dev, 8) || misaligned(workspace_dev, 8))
    return fail(TB_E_INVAL, "tb_trpo_returns: idx, count and the workspace must be 8-byte aligned");
  size_t rs, ds;
  if (int rc = step_strides("tb_trpo_returns", n_envs, reward_step_stride_bytes, done_step_stride_bytes, &rs, &ds)) return rc;
  if ((long long)n_steps * trpo_return_chunks(n_envs) > 0x7fffffffLL) return fail(TB_E_INVAL, "tb_trpo_returns: n_steps * ceil(n_envs / 64) must be below 2^31");
  if ((long long)workspace_bytes < tb_trpo_returns_workspace_bytes(n_steps, n_envs))
    return fail(TB_E_INVAL, "tb_trpo_returns: the workspace is smaller than tb_trpo_returns_workspace_bytes");
  DeviceGuard g;
  if (int rc = learner_device(g, device, "tb_trpo_returns")) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int chunks = (int)trpo_return_chunks(n_envs);
  const long long entries = (long long)n_steps * chunks;
  long long* table = (long long*)workspace_dev;
  int* last = (int*)(table + entries);
  const dim3 waves((unsigned)((entries + 3) / 4));
  if (int rc = launch(tb_trpo_returns_kernel, dim3((unsigned)chunks), dim3(64), 0, s, n_steps, n_envs, rewards_dev, rs, dones_dev, ds, discount, returns_dev, last)) return rc;
  if (int rc = launch(tb_trpo_finished_count_kernel, waves, dim3(256), 0, s, n_steps, n_envs, chunks, (const int*)last, table)) return rc;
  if (int rc = launch(tb_trpo_finished_scan_kernel, dim3(1), dim3(1024), 0, s, entries, table, (long long*)count_dev)) return rc;
  return launch(tb_trpo_finished_scatter_kernel, waves, dim3(256), 0, s, n_steps, n_envs, chunks, (const int*)last, (const long long*)table, (long long*)idx_dev);
}

// --------------------------------------------------------------------------------------------- the SAC and TQC learners (tb_sac.hpp, tb_tqc.hpp)
// Every stage is written once, as a template over an algorithm descriptor (SacAlgo, TqcAlgo); the C entry points forward to it.
extern "C++" {
namespace {
struct SacDims {  // SacLayout<KIND> at run time
  int O, A, C, pi_w0, pi_b0, pi_w1, pi_b1, pi_head, pi_block, pi_p, q_w0, q_b0, q_w1, q_b1, q_w2, q_b2, q_one, q_p;
};
template <int KIND> SacDims sac_dims_of() {
  using L = SacLayout<KIND>;
  return {L::O, L::A, L::C, L::PI_W0, L::PI_B0, L::PI_W1, L::PI_B1, L::PI_HEAD, L::PI_HEAD_BLOCK, L::PI_P, L::Q_W0, L::Q_B0, L::Q_W1, L::Q_B1, L::Q_W2, L::Q_B2, L::Q_ONE, L::Q_P};
}
// TQC: SAC's dims with the critic's 25-wide last layer
template <int KIND> SacDims tqc_dims_of() {
  using L = TqcLayout<KIND>;
  SacDims d = sac_dims_of<KIND>();
  d.q_w2 = L::Q_W2; d.q_b2 = L::Q_B2; d.q_one = L::Q_ONE; d.q_p = L::Q_P;
  return d;
}

unsigned sac_blocks(long long n, int per) { return (unsigned)((n + per - 1) / per); }

// A population's rows (tb_sac_*_members; null: one learner): strides in entries (idx) and floats, zero where a stage has no such array
struct SacPop {
  int M;
  size_t idx, pi, q, eps, act, logp, y;
  const TbSacMemberHp* hp;
};

struct SacRun {  // one stage's launches: the dims, the stream, the batch and the workspace's regions
  SacDims d;
  hipStream_t s;
  int B;
  float* ws;
  int heads, hw;  // a critic's outputs and the padded width of its head rows: 1 / 16 for SAC, 25 / 32 for TQC
  // a population: the members' count, the row strides of the workspace regions, the actor and the critic (floats), and what the
  // row kernels take. One learner: pop is false, NM is 1, and every launch below is the launch it was.
  bool pop;
  int NM;
  long long wss, pis, qs;
  SacRowMembers rm;
  float* at(int region) const { return ws + (size_t)region * (size_t)B; }  // (of member 0: the kernels add the member's region)

  // ps: the row stride of the flat vector that holds w (pis or qs)
  int forward(bool relu, const float* x, int xs, long long xz, const float* w, int wrs, long long wz, const float* bias, float* y, int ys, long long yz, int K, int M, int nets,
              long long ps) const {
    SacFwdArgs a = {x, xs, xz, w, wrs, wz, bias, y, ys, yz, B, K, M};
    const dim3 grid(sac_blocks(B, SAC_ROWS_PER_WG), sac_blocks(M, 16), (unsigned)(nets * NM));
    if (pop) {
      const SacMembers mb = {nets, wss, ps};
      return relu ? launch(sac_forward_kernel<true, SacMembers>, grid, dim3(256), 0, s, a, mb) : launch(sac_forward_kernel<false, SacMembers>, grid, dim3(256), 0, s, a, mb);
    }
    return relu ? launch(sac_forward_kernel<true>, grid, dim3(256), 0, s, a) : launch(sac_forward_kernel<false>, grid, dim3(256), 0, s, a);
  }
  int backward(const float* dz, int dzs, long long dzz, const float* w, int wrs, long long wz, int split, int extra, const float* h, int hs, long long hz, float* dx, int dxs,
               long long dxz, int K, int M, int nets, long long ps) const {
    SacBwdArgs a = {dz, dzs, dzz, w, wrs, wz, split, extra, h, hs, hz, dx, dxs, dxz, B, K, M};
    const dim3 grid(sac_blocks(B, SAC_ROWS_PER_WG), sac_blocks(K, 16), (unsigned)(nets * NM));
    if (pop) {
      const SacMembers mb = {nets, wss, ps};
      return h ? launch(sac_backward_kernel<true, SacMembers>, grid, dim3(256), 0, s, a, mb) : launch(sac_backward_kernel<false, SacMembers>, grid, dim3(256), 0, s, a, mb);
    }
    return h ? launch(sac_backward_kernel<true>, grid, dim3(256), 0, s, a) : launch(sac_backward_kernel<false>, grid, dim3(256), 0, s, a);
  }
  int wgrad(const float* dz, int dzs, long long dzz, const float* h, int hs, long long hz, float* gw, int wrs, long long wz, float* gb, int K, int M, int nets, long long ps) const {
    SacWgradArgs a = {dz, dzs, dzz, h, hs, hz, gw, wrs, wz, gb, B, K, M};
    const dim3 grid(sac_blocks(K, 64), sac_blocks(M, 16), (unsigned)(nets * NM));
    if (pop) {
      const SacMembers mb = {nets, wss, ps};
      return launch(sac_wgrad_kernel<SacMembers>, grid, dim3(256), 0, s, a, mb);
    }
    return launch(sac_wgrad_kernel<>, grid, dim3(256), 0, s, a);
  }
  // a row kernel or a one-workgroup reduction: k1 for one learner; km for a population, the member as grid axis y (member_is_x: x)
  template <class... P1, class... PM, class... A>
  int rows(void (*k1)(P1...), void (*km)(PM...), dim3 grid, bool member_is_x, const A&... a) const {
    if (!pop) return launch(k1, grid, dim3(256), 0, s, a...);
    if (member_is_x) grid.x = (unsigned)NM;
    else grid.y = (unsigned)NM;
    return launch(km, grid, dim3(256), 0, s, a..., rm);
  }
  // rows idx of obs, and of action beside them where there is one, into the 16-wide rows of region x
  int gather(const float* obs, const float* action, const int64_t* idx, long long n_rows, int x) const {
    return rows(sac_gather_kernel<>, sac_gather_kernel<SacRowMembers>, dim3(sac_blocks((long long)B * 16, 256)), false, obs, d.O, action, action ? d.A : 0, (const long long*)idx,
                n_rows, B, at(x));
  }
  // the actor on the gathered rows x0: h1, h2, the head's outputs zh; then the sample: act / logp out, xc = obs | sample, lp
  int actor(const float* actor, const float* eps, int x0, int h1, int h2, int zh, int xc, int lp, float* act_out, float* logp_out) const {
    if (int rc = forward(true, at(x0), SAC_XW, 0, actor + d.pi_w0, d.O, 0, actor + d.pi_b0, at(h1), SAC_H, 0, d.O, SAC_H, 1, pis)) return rc;
    if (int rc = forward(true, at(h1), SAC_H, 0, actor + d.pi_w1, SAC_H, 0, actor + d.pi_b1, at(h2), SAC_H, 0, SAC_H, SAC_H, 1, pis)) return rc;
    if (int rc = forward(false, at(h2), SAC_H, 0, actor + d.pi_head, SAC_H, d.pi_block, actor + d.pi_head + d.A * SAC_H, at(zh), SAC_XW, d.A, SAC_H, d.A, 2, pis)) return rc;
    return rows(sac_sample_kernel<>, sac_sample_kernel<SacRowMembers>, dim3(sac_blocks(B, 256)), false, (const float*)at(x0), (const float*)at(zh), eps, d.O, d.A, B, act_out,
                logp_out, at(xc), at(lp));
  }
  // both nets of a critic vector on the rows xc: h1, h2 [2][B][256], q [2][B][hw] (columns 0 .. heads)
  int critics(const float* critic, int xc, int h1, int h2, int q) const {
    const long long BH = (long long)B * SAC_H;
    if (int rc = forward(true, at(xc), SAC_XW, 0, critic + d.q_w0, d.C, d.q_one, critic + d.q_b0, at(h1), SAC_H, BH, d.C, SAC_H, 2, qs)) return rc;
    if (int rc = forward(true, at(h1), SAC_H, BH, critic + d.q_w1, SAC_H, d.q_one, critic + d.q_b1, at(h2), SAC_H, BH, SAC_H, SAC_H, 2, qs)) return rc;
    return forward(false, at(h2), SAC_H, BH, critic + d.q_w2, SAC_H, d.q_one, critic + d.q_b2, at(q), hw, (long long)B * hw, SAC_H, heads, 2, qs);
  }
  // dq [2][B][hw] back to dz2 and dz1 [2][B][256] through both nets, in the regions of the workspace layout Ws
  template <class Ws> int critics_backward(const float* critic) const {
    const long long BH = (long long)B * SAC_H;
    if (int rc = backward(at(Ws::DQ), hw, (long long)B * hw, critic + d.q_w2, SAC_H, d.q_one, 1 << 30, 0, at(Ws::C2), SAC_H, BH, at(Ws::DZ2), SAC_H, BH, SAC_H, heads, 2, qs)) return rc;
    return backward(at(Ws::DZ2), SAC_H, BH, critic + d.q_w1, SAC_H, d.q_one, 1 << 30, 0, at(Ws::C1), SAC_H, BH, at(Ws::DZ1), SAC_H, BH, SAC_H, SAC_H, 2, qs);
  }
};

// What is an algorithm's own in a stage: its layouts, a critic's head count and padded head width, the name of its workspace
// query, and the launches of its targets and its two losses. The target and actor-loss kernels of both take the same arguments,
// which the stage lists; the critic loss is one launch in SAC and two in TQC (the rows' sums into RL, then their sum).
struct SacAlgo {
  using Ws = SacWs;
  static constexpr int HEADS = 1, HW = SAC_XW, Y_W = 1;  // Y_W: the floats of a row's target
  static constexpr const char* WS_QUERY = "tb_sac_workspace_bytes";
  static SacDims dims(int env_kind) { return env_kind == TB_ENV_SWING ? sac_dims_of<TB_ENV_SWING>() : sac_dims_of<TB_ENV_TENNIS>(); }
  template <class... A> static int targets(const SacRun& r, const A&... a) {
    return r.rows(sac_target_kernel<>, sac_target_kernel<SacRowMembers>, dim3(sac_blocks(r.B, 256)), false, a...);
  }
  static int critic_loss(const SacRun& r, const float* y, double* stats) {
    return r.rows(sac_critic_loss_kernel<>, sac_critic_loss_kernel<SacRowMembers>, dim3(1), true, (const float*)r.at(Ws::Q), y, r.B, r.at(Ws::DQ), stats);
  }
  template <class... A> static int actor_loss(const SacRun& r, const A&... a) {  // the critics' min
    return r.rows(sac_actor_loss_kernel<>, sac_actor_loss_kernel<SacRowMembers>, dim3(1), true, a...);
  }
};
struct TqcAlgo {
  using Ws = TqcWs;
  static constexpr int HEADS = TQC_Q, HW = TQC_HW, Y_W = TQC_KEEP;
  static constexpr const char* WS_QUERY = "tb_tqc_workspace_bytes";
  static SacDims dims(int env_kind) { return env_kind == TB_ENV_SWING ? tqc_dims_of<TB_ENV_SWING>() : tqc_dims_of<TB_ENV_TENNIS>(); }
  template <class... A> static int targets(const SacRun& r, const A&... a) {
    return r.rows(tqc_target_kernel<>, tqc_target_kernel<SacRowMembers>, dim3(sac_blocks(r.B, 4)), false, a...);
  }
  static int critic_loss(const SacRun& r, const float* y, double* stats) {
    double* row_loss = reinterpret_cast<double*>(r.at(Ws::RL));
    if (int rc = r.rows(tqc_critic_loss_kernel<>, tqc_critic_loss_kernel<SacRowMembers>, dim3(sac_blocks(r.B, 4)), false, (const float*)r.at(Ws::Q), y, r.B, r.at(Ws::DQ), row_loss))
      return rc;
    return r.rows(tqc_loss_sum_kernel<>, tqc_loss_sum_kernel<SacRowMembers>, dim3(1), true, (const double*)row_loss, r.B, stats);
  }
  template <class... A> static int actor_loss(const SacRun& r, const A&... a) {  // their 50 quantiles' mean
    return r.rows(tqc_actor_loss_kernel<>, tqc_actor_loss_kernel<SacRowMembers>, dim3(1), true, a...);
  }
};

int sac_fail(int code, const char* what, const char* words, const char* more = "") {
  char msg[192];
  snprintf(msg, sizeof msg, "%s: %s%s", what, words, more);
  return fail(code, msg);
}

// What a stage refuses before its first launch, in this order: the env kind, the batch and the workspace; null pointers;
// n_rows; alignment (wide8 names what must be 8-byte aligned); aliasing (aliased: the words of the refusal, or null); the device, which
// g then makes current for the rest of the stage. A population (pop: not null) adds its member count in front of the batch, asks
// for n_members workspace regions, and refuses a stride shorter than what it strides over (short_stride: the stage's own verdict).
template <class Algo> long long sac_members_workspace_stride(int batch) {
  return ((long long)sizeof(float) * Algo::Ws::PER_ROW * (long long)batch + 7) / 8 * 8;
}
template <class Algo>
int sac_check(const char* what, int env_kind, int batch, const void* workspace_dev, size_t workspace_bytes, bool any_null, long long n_rows, bool any_misaligned,
              const char* wide8, const char* aliased, int device, DeviceGuard& g, const SacPop* pop = nullptr, bool short_stride = false) {
  if (!kind_ok(env_kind)) return sac_fail(TB_E_INVAL, what, "unknown env kind");
  if (pop && (pop->M < 1 || pop->M > TB_SAC_MAX_MEMBERS)) return sac_fail(TB_E_INVAL, what, "n_members must be in [1, 32767] (member and net share the grid's z axis)");
  if (batch < 1) return sac_fail(TB_E_INVAL, what, "batch must be >= 1");
  if (!workspace_dev) return sac_fail(TB_E_INVAL, what, "null argument (the workspace)");
  if (misaligned(workspace_dev, 8)) return sac_fail(TB_E_INVAL, what, "the workspace must be 8-byte aligned");
  if (pop) {
    if ((long long)(workspace_bytes / (size_t)pop->M) < sac_members_workspace_stride<Algo>(batch))
      return sac_fail(TB_E_PARAMS, what, "the workspace is smaller than n_members regions of the members_workspace_stride_bytes query");
  } else if ((long long)workspace_bytes < (long long)sizeof(float) * Algo::Ws::PER_ROW * (long long)batch) {
    return sac_fail(TB_E_PARAMS, what, "the workspace is smaller than ", Algo::WS_QUERY);
  }
  if (any_null) return sac_fail(TB_E_INVAL, what, "null argument");
  if (n_rows < 1) return sac_fail(TB_E_INVAL, what, "n_rows must be >= 1");
  if (any_misaligned) return sac_fail(TB_E_INVAL, what, "a float array is not 4-byte aligned, or ", wide8);
  if (short_stride) return sac_fail(TB_E_INVAL, what, "a member stride is shorter than the row it strides over");
  if (aliased) return sac_fail(TB_E_INVAL, what, aliased);
  return learner_device(g, device, what);
}
template <class Algo> SacRun sac_run(int env_kind, void* stream, int batch, void* workspace_dev, const SacPop* pop) {
  SacRun r = {Algo::dims(env_kind), (hipStream_t)stream, batch, (float*)workspace_dev, Algo::HEADS, Algo::HW, false, 1, 0, 0, 0, {}};
  if (pop) {
    r.pop = true; r.NM = pop->M;
    r.wss = sac_members_workspace_stride<Algo>(batch) / (long long)sizeof(float);
    r.pis = (long long)pop->pi; r.qs = (long long)pop->q;
    r.rm = {(long long)pop->idx, (long long)pop->eps, (long long)pop->act, (long long)pop->logp, (long long)pop->y, r.wss, pop->hp};
  }
  return r;
}
// the dims of a kind that may be unknown (then zeros: sac_check refuses the kind first)
template <class Algo> SacDims sac_dims_or_zero(int env_kind) { return kind_ok(env_kind) ? Algo::dims(env_kind) : SacDims{}; }
// a population's rows [M] of n floats, `stride` apart, from a and from b: do the two ranges share a float?
bool sac_rows_overlap(const float* a, const float* b, size_t stride, int M, long long n) {
  const uintptr_t span = ((uintptr_t)(M - 1) * stride + (uintptr_t)n) * sizeof(float), pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + span && pb < pa + span;
}

template <class Algo> int sac_param_floats(const char* what, int env_kind, int which) {
  if (!kind_ok(env_kind)) return sac_fail(TB_E_INVAL, what, "unknown env kind");
  if (which != TB_SAC_ACTOR && which != TB_SAC_CRITIC) return sac_fail(TB_E_INVAL, what, "which must be TB_SAC_ACTOR or TB_SAC_CRITIC");
  const SacDims d = Algo::dims(env_kind);
  return which == TB_SAC_ACTOR ? d.pi_p : d.q_p;
}
template <class Algo> long long sac_workspace_bytes(const char* what, int env_kind, int batch) {
  if (!kind_ok(env_kind) || batch < 1) return sac_fail(TB_E_INVAL, what, "unknown env kind, or batch < 1");
  return (long long)sizeof(float) * Algo::Ws::PER_ROW * (long long)batch;
}

template <class Algo>
int sac_actor_forward(const char* what, int env_kind, int device, void* stream, const float* obs_dev, long long n_rows, const int64_t* idx_dev, int batch, const float* actor_dev,
                      const float* eps_dev, float* act_out_dev, float* logp_out_dev, void* workspace_dev, size_t workspace_bytes, const SacPop* pop = nullptr) {
  using Ws = typename Algo::Ws;
  DeviceGuard g;
  const SacDims d0 = sac_dims_or_zero<Algo>(env_kind);
  const size_t BA = (size_t)batch * (size_t)d0.A;
  if (int rc = sac_check<Algo>(what, env_kind, batch, workspace_dev, workspace_bytes, !obs_dev || !idx_dev || !actor_dev || !eps_dev || !act_out_dev || !logp_out_dev, n_rows,
                               misaligned(obs_dev, 4) || misaligned(actor_dev, 4) || misaligned(eps_dev, 4) || misaligned(act_out_dev, 4) || misaligned(logp_out_dev, 4) ||
                                   misaligned(idx_dev, 8),
                               "idx not 8-byte aligned", nullptr, device, g, pop,
                               pop && (pop->idx < (size_t)batch || pop->pi < (size_t)d0.pi_p || pop->eps < BA || pop->act < BA || pop->logp < (size_t)batch)))
    return rc;
  const SacRun r = sac_run<Algo>(env_kind, stream, batch, workspace_dev, pop);
  if (int rc = r.gather(obs_dev, nullptr, idx_dev, n_rows, Ws::X0)) return rc;
  return r.actor(actor_dev, eps_dev, Ws::X0, Ws::H1, Ws::H2, Ws::ZH, Ws::XC, Ws::LP, act_out_dev, logp_out_dev);
}

template <class Algo>
int sac_targets(const char* what, int env_kind, int device, void* stream, const float* next_obs_dev, const float* reward_dev, const float* done_dev, long long n_rows,
                const int64_t* idx_dev, int batch, const float* actor_dev, const float* target_dev, const float* log_ent_coef_dev, const float* eps_next_dev, float gamma,
                float* y_dev, void* workspace_dev, size_t workspace_bytes, const SacPop* pop = nullptr) {
  using Ws = typename Algo::Ws;
  DeviceGuard g;
  const SacDims d0 = sac_dims_or_zero<Algo>(env_kind);
  if (int rc = sac_check<Algo>(what, env_kind, batch, workspace_dev, workspace_bytes,
                               !next_obs_dev || !reward_dev || !done_dev || !idx_dev || !actor_dev || !target_dev || !log_ent_coef_dev || !eps_next_dev || !y_dev ||
                                   (pop && !pop->hp),
                               n_rows,
                               misaligned(next_obs_dev, 4) || misaligned(reward_dev, 4) || misaligned(done_dev, 4) || misaligned(actor_dev, 4) || misaligned(target_dev, 4) ||
                                   misaligned(log_ent_coef_dev, 4) || misaligned(eps_next_dev, 4) || misaligned(y_dev, 4) || misaligned(idx_dev, 8) ||
                                   (pop && misaligned(pop->hp, 8)),
                               pop ? "idx / hp not 8-byte aligned" : "idx not 8-byte aligned", nullptr, device, g, pop,
                               pop && (pop->idx < (size_t)batch || pop->pi < (size_t)d0.pi_p || pop->q < (size_t)d0.q_p || pop->eps < (size_t)batch * (size_t)d0.A ||
                                       pop->y < (size_t)batch * (size_t)Algo::Y_W)))
    return rc;
  const SacRun r = sac_run<Algo>(env_kind, stream, batch, workspace_dev, pop);
  if (int rc = r.gather(next_obs_dev, nullptr, idx_dev, n_rows, Ws::NX0)) return rc;
  if (int rc = r.actor(actor_dev, eps_next_dev, Ws::NX0, Ws::NH1, Ws::NH2, Ws::NZH, Ws::NXC, Ws::NAL, nullptr, nullptr)) return rc;  // logp' in NAL
  if (int rc = r.critics(target_dev, Ws::NXC, Ws::T1, Ws::T2, Ws::QT)) return rc;
  return Algo::targets(r, reward_dev, done_dev, (const long long*)idx_dev, n_rows, batch, (const float*)r.at(Ws::QT), (const float*)r.at(Ws::NAL), log_ent_coef_dev, gamma, y_dev);
}

template <class Algo>
int sac_critic_grad(const char* what, int env_kind, int device, void* stream, const float* obs_dev, const float* action_dev, long long n_rows, const int64_t* idx_dev, int batch,
                    const float* critic_dev, const float* y_dev, float* grad_dev, double* stats_dev, void* workspace_dev, size_t workspace_bytes, const SacPop* pop = nullptr) {
  using Ws = typename Algo::Ws;
  DeviceGuard g;
  const SacDims d0 = sac_dims_or_zero<Algo>(env_kind);
  const char* aliased = grad_dev == critic_dev ? "grad_dev must not be critic_dev" : nullptr;
  if (pop && pop->M >= 1 && grad_dev && critic_dev && sac_rows_overlap(grad_dev, critic_dev, pop->q, pop->M, d0.q_p)) aliased = "the rows of grad_dev overlap the rows of critic_dev";
  if (int rc = sac_check<Algo>(what, env_kind, batch, workspace_dev, workspace_bytes, !obs_dev || !action_dev || !idx_dev || !critic_dev || !y_dev || !grad_dev || !stats_dev, n_rows,
                               misaligned(obs_dev, 4) || misaligned(action_dev, 4) || misaligned(critic_dev, 4) || misaligned(y_dev, 4) || misaligned(grad_dev, 4) ||
                                   misaligned(idx_dev, 8) || misaligned(stats_dev, 8),
                               "idx / stats not 8-byte aligned", aliased, device, g, pop,
                               pop && (pop->idx < (size_t)batch || pop->q < (size_t)d0.q_p || pop->y < (size_t)batch * (size_t)Algo::Y_W)))
    return rc;
  const SacRun r = sac_run<Algo>(env_kind, stream, batch, workspace_dev, pop);
  const SacDims& d = r.d;
  const long long BH = (long long)batch * SAC_H;
  if (int rc = r.gather(obs_dev, action_dev, idx_dev, n_rows, Ws::XSA)) return rc;
  if (int rc = r.critics(critic_dev, Ws::XSA, Ws::C1, Ws::C2, Ws::Q)) return rc;
  if (int rc = Algo::critic_loss(r, y_dev, stats_dev)) return rc;
  if (int rc = r.template critics_backward<Ws>(critic_dev)) return rc;
  if (int rc = r.wgrad(r.at(Ws::DQ), r.hw, (long long)batch * r.hw, r.at(Ws::C2), SAC_H, BH, grad_dev + d.q_w2, SAC_H, d.q_one, grad_dev + d.q_b2, SAC_H, r.heads, 2, r.qs)) return rc;
  if (int rc = r.wgrad(r.at(Ws::DZ2), SAC_H, BH, r.at(Ws::C1), SAC_H, BH, grad_dev + d.q_w1, SAC_H, d.q_one, grad_dev + d.q_b1, SAC_H, SAC_H, 2, r.qs)) return rc;
  return r.wgrad(r.at(Ws::DZ1), SAC_H, BH, r.at(Ws::XSA), SAC_XW, 0, grad_dev + d.q_w0, d.C, d.q_one, grad_dev + d.q_b0, d.C, SAC_H, 2, r.qs);
}

template <class Algo>
int sac_actor_grad(const char* what, int env_kind, int device, void* stream, int batch, const float* actor_dev, const float* critic_dev, const float* log_ent_coef_dev,
                   const float* eps_dev, float* actor_grad_dev, float* ent_grad_dev, double* stats_dev, void* workspace_dev, size_t workspace_bytes, const SacPop* pop = nullptr) {
  using Ws = typename Algo::Ws;
  DeviceGuard g;
  const SacDims d0 = sac_dims_or_zero<Algo>(env_kind);
  const char* aliased = actor_grad_dev == actor_dev ? "actor_grad_dev must not be actor_dev" : nullptr;
  if (pop && pop->M >= 1 && actor_grad_dev && actor_dev && sac_rows_overlap(actor_grad_dev, actor_dev, pop->pi, pop->M, d0.pi_p))
    aliased = "the rows of actor_grad_dev overlap the rows of actor_dev";
  if (int rc = sac_check<Algo>(what, env_kind, batch, workspace_dev, workspace_bytes,
                               !actor_dev || !critic_dev || !log_ent_coef_dev || !eps_dev || !actor_grad_dev || !ent_grad_dev || !stats_dev, 1,
                               misaligned(actor_dev, 4) || misaligned(critic_dev, 4) || misaligned(log_ent_coef_dev, 4) || misaligned(eps_dev, 4) || misaligned(actor_grad_dev, 4) ||
                                   misaligned(ent_grad_dev, 4) || misaligned(stats_dev, 8),
                               "stats not 8-byte aligned", aliased, device, g, pop,
                               pop && (pop->pi < (size_t)d0.pi_p || pop->q < (size_t)d0.q_p || pop->eps < (size_t)batch * (size_t)d0.A)))
    return rc;
  const SacRun r = sac_run<Algo>(env_kind, stream, batch, workspace_dev, pop);
  const SacDims& d = r.d;
  const long long BH = (long long)batch * SAC_H, BX = (long long)batch * SAC_XW;
  // the critics as they are now on (s, a~), the algorithm's statistic of them, and back to their input
  if (int rc = r.critics(critic_dev, Ws::XC, Ws::C1, Ws::C2, Ws::Q)) return rc;
  if (int rc = Algo::actor_loss(r, (const float*)r.at(Ws::Q), (const float*)r.at(Ws::LP), log_ent_coef_dev, -(float)d.A, batch, r.at(Ws::DQ), ent_grad_dev, stats_dev)) return rc;
  if (int rc = r.template critics_backward<Ws>(critic_dev)) return rc;
  if (int rc = r.backward(r.at(Ws::DZ1), SAC_H, BH, critic_dev + d.q_w0, d.C, d.q_one, 1 << 30, 0, nullptr, 0, 0, r.at(Ws::DX), SAC_XW, BX, d.C, SAC_H, 2, r.qs)) return rc;
  // through tanh and logp to the head's outputs, then the actor's own backward pass
  if (int rc = r.rows(sac_head_backward_kernel<>, sac_head_backward_kernel<SacRowMembers>, dim3(sac_blocks((long long)batch * 16, 256)), false, (const float*)r.at(Ws::ZH),
                      (const float*)r.at(Ws::XC), (const float*)r.at(Ws::DX), eps_dev, log_ent_coef_dev, d.O, d.A, batch, r.at(Ws::DHD)))
    return rc;
  float* gh = actor_grad_dev + d.pi_head;
  if (int rc = r.wgrad(r.at(Ws::DHD), SAC_XW, d.A, r.at(Ws::H2), SAC_H, 0, gh, SAC_H, d.pi_block, gh + d.A * SAC_H, SAC_H, d.A, 2, r.pis)) return rc;
  if (int rc = r.backward(r.at(Ws::DHD), SAC_XW, 0, actor_dev + d.pi_head, SAC_H, 0, d.A, d.A, r.at(Ws::H2), SAC_H, 0, r.at(Ws::DA2), SAC_H, 0, SAC_H, 2 * d.A, 1, r.pis)) return rc;
  if (int rc = r.wgrad(r.at(Ws::DA2), SAC_H, 0, r.at(Ws::H1), SAC_H, 0, actor_grad_dev + d.pi_w1, SAC_H, 0, actor_grad_dev + d.pi_b1, SAC_H, SAC_H, 1, r.pis)) return rc;
  if (int rc = r.backward(r.at(Ws::DA2), SAC_H, 0, actor_dev + d.pi_w1, SAC_H, 0, 1 << 30, 0, r.at(Ws::H1), SAC_H, 0, r.at(Ws::DA1), SAC_H, 0, SAC_H, SAC_H, 1, r.pis)) return rc;
  return r.wgrad(r.at(Ws::DA1), SAC_H, 0, r.at(Ws::X0), SAC_XW, 0, actor_grad_dev + d.pi_w0, d.O, 0, actor_grad_dev + d.pi_b0, d.O, SAC_H, 1, r.pis);
}
template <class Algo> long long sac_members_workspace_stride_bytes(const char* what, int env_kind, int batch) {
  if (!kind_ok(env_kind) || batch < 1) return sac_fail(TB_E_INVAL, what, "unknown env kind, or batch < 1");
  return sac_members_workspace_stride<Algo>(batch);
}
}  // namespace
}  // extern "C++"

int tb_sac_param_floats(int env_kind, int which) { return sac_param_floats<SacAlgo>(__func__, env_kind, which); }
int tb_tqc_param_floats(int env_kind, int which) { return sac_param_floats<TqcAlgo>(__func__, env_kind, which); }
int tb_sac_rows_per_workgroup(void) { return SAC_ROWS_PER_WG; }
long long tb_sac_workspace_bytes(int env_kind, int batch) { return sac_workspace_bytes<SacAlgo>(__func__, env_kind, batch); }
long long tb_tqc_workspace_bytes(int env_kind, int batch) { return sac_workspace_bytes<TqcAlgo>(__func__, env_kind, batch); }

int tb_sac_actor_forward(int env_kind, int device, void* stream, const float* obs_dev, long long n_rows, const int64_t* idx_dev, int batch, const float* actor_dev,
                         const float* eps_dev, float* act_out_dev, float* logp_out_dev, void* workspace_dev, size_t workspace_bytes) {
  return sac_actor_forward<SacAlgo>(__func__, env_kind, device, stream, obs_dev, n_rows, idx_dev, batch, actor_dev, eps_dev, act_out_dev, logp_out_dev, workspace_dev, workspace_bytes);
}
int tb_tqc_actor_forward(int env_kind, int device, void* stream, const float* obs_dev, long long n_rows, const int64_t* idx_dev, int batch, const float* actor_dev,
                         const float* eps_dev, float* act_out_dev, float* logp_out_dev, void* workspace_dev, size_t workspace_bytes) {
  return sac_actor_forward<TqcAlgo>(__func__, env_kind, device, stream, obs_dev, n_rows, idx_dev, batch, actor_dev, eps_dev, act_out_dev, logp_out_dev, workspace_dev, workspace_bytes);
}

int tb_sac_targets(int env_kind, int device, void* stream, const float* next_obs_dev, const float* reward_dev, const float* done_dev, long long n_rows,
                   const int64_t* idx_dev, int batch, const float* actor_dev, const float* target_dev, const float* log_ent_coef_dev, const float* eps_next_dev,
                   float gamma, float* y_dev, void* workspace_dev, size_t workspace_bytes) {
  return sac_targets<SacAlgo>(__func__, env_kind, device, stream, next_obs_dev, reward_dev, done_dev, n_rows, idx_dev, batch, actor_dev, target_dev, log_ent_coef_dev, eps_next_dev,
                              gamma, y_dev, workspace_dev, workspace_bytes);
}
int tb_tqc_targets(int env_kind, int device, void* stream, const float* next_obs_dev, const float* reward_dev, const float* done_dev, long long n_rows,
                   const int64_t* idx_dev, int batch, const float* actor_dev, const float* target_dev, const float* log_ent_coef_dev, const float* eps_next_dev,
                   float gamma, float* y_dev, void* workspace_dev, size_t workspace_bytes) {
  return sac_targets<TqcAlgo>(__func__, env_kind, device, stream, next_obs_dev, reward_dev, done_dev, n_rows, idx_dev, batch, actor_dev, target_dev, log_ent_coef_dev, eps_next_dev,
                              gamma, y_dev, workspace_dev, workspace_bytes);
}

int tb_sac_critic_grad(int env_kind, int device, void* stream, const float* obs_dev, const float* action_dev, long long n_rows, const int64_t* idx_dev, int batch,
                       const float* critic_dev, const float* y_dev, float* grad_dev, double* stats_dev, void* workspace_dev, size_t workspace_bytes) {
  return sac_critic_grad<SacAlgo>(__func__, env_kind, device, stream, obs_dev, action_dev, n_rows, idx_dev, batch, critic_dev, y_dev, grad_dev, stats_dev, workspace_dev, workspace_bytes);
}
int tb_tqc_critic_grad(int env_kind, int device, void* stream, const float* obs_dev, const float* action_dev, long long n_rows, const int64_t* idx_dev, int batch,
                       const float* critic_dev, const float* y_dev, float* grad_dev, double* stats_dev, void* workspace_dev, size_t workspace_bytes) {
  return sac_critic_grad<TqcAlgo>(__func__, env_kind, device, stream, obs_dev, action_dev, n_rows, idx_dev, batch, critic_dev, y_dev, grad_dev, stats_dev, workspace_dev, workspace_bytes);
}

int tb_sac_actor_grad(int env_kind, int device, void* stream, int batch, const float* actor_dev, const float* critic_dev, const float* log_ent_coef_dev, const float* eps_dev,
                      float* actor_grad_dev, float* ent_grad_dev, double* stats_dev, void* workspace_dev, size_t workspace_bytes) {
  return sac_actor_grad<SacAlgo>(__func__, env_kind, device, stream, batch, actor_dev, critic_dev, log_ent_coef_dev, eps_dev, actor_grad_dev, ent_grad_dev, stats_dev, workspace_dev,
                                 workspace_bytes);
}
int tb_tqc_actor_grad(int env_kind, int device, void* stream, int batch, const float* actor_dev, const float* critic_dev, const float* log_ent_coef_dev, const float* eps_dev,
                      float* actor_grad_dev, float* ent_grad_dev, double* stats_dev, void* workspace_dev, size_t workspace_bytes) {
  return sac_actor_grad<TqcAlgo>(__func__, env_kind, device, stream, batch, actor_dev, critic_dev, log_ent_coef_dev, eps_dev, actor_grad_dev, ent_grad_dev, stats_dev, workspace_dev,
                                 workspace_bytes);
}

// ---- the population's entry points: the same bodies with a SacPop
#define TB_SAC_MEMBERS_ENTRIES(PREFIX, ALGO)                                                                                                                                   \
  long long PREFIX##members_workspace_stride_bytes(int env_kind, int batch) { return sac_members_workspace_stride_bytes<ALGO>(__func__, env_kind, batch); }                   \
  int PREFIX##actor_forward_members(int env_kind, int device, void* stream, const float* obs_dev, long long n_rows, const int64_t* idx_dev, size_t idx_stride, int batch,       \
                                    int n_members, const float* actor_dev, size_t actor_stride_floats, const float* eps_dev, size_t eps_stride_floats, float* act_out_dev,      \
                                    size_t act_stride_floats, float* logp_out_dev, size_t logp_stride_floats, void* workspace_dev, size_t workspace_bytes) {                    \
    const SacPop pop = {n_members, idx_stride, actor_stride_floats, 0, eps_stride_floats, act_stride_floats, logp_stride_floats, 0, nullptr};                                   \
    return sac_actor_forward<ALGO>(__func__, env_kind, device, stream, obs_dev, n_rows, idx_dev, batch, actor_dev, eps_dev, act_out_dev, logp_out_dev, workspace_dev,          \
                                   workspace_bytes, &pop);                                                                                                                      \
  }                                                                                                                                                                             \
  int PREFIX##targets_members(int env_kind, int device, void* stream, const float* next_obs_dev, const float* reward_dev, const float* done_dev, long long n_rows,             \
                              const int64_t* idx_dev, size_t idx_stride, int batch, int n_members, const float* actor_dev, size_t actor_stride_floats, const float* target_dev, \
                              size_t critic_stride_floats, const float* log_ent_coef_dev, const float* eps_next_dev, size_t eps_stride_floats, const TbSacMemberHp* hp_dev,     \
                              float* y_dev, size_t y_stride_floats, void* workspace_dev, size_t workspace_bytes) {                                                              \
    const SacPop pop = {n_members, idx_stride, actor_stride_floats, critic_stride_floats, eps_stride_floats, 0, 0, y_stride_floats, hp_dev};                                    \
    return sac_targets<ALGO>(__func__, env_kind, device, stream, next_obs_dev, reward_dev, done_dev, n_rows, idx_dev, batch, actor_dev, target_dev, log_ent_coef_dev,          \
                             eps_next_dev, 0.0f, y_dev, workspace_dev, workspace_bytes, &pop);                                                                                  \
  }                                                                                                                                                                             \
  int PREFIX##critic_grad_members(int env_kind, int device, void* stream, const float* obs_dev, const float* action_dev, long long n_rows, const int64_t* idx_dev,             \
                                  size_t idx_stride, int batch, int n_members, const float* critic_dev, size_t critic_stride_floats, const float* y_dev,                        \
                                  size_t y_stride_floats, float* grad_dev, double* stats_dev, void* workspace_dev, size_t workspace_bytes) {                                    \
    const SacPop pop = {n_members, idx_stride, 0, critic_stride_floats, 0, 0, 0, y_stride_floats, nullptr};                                                                     \
    return sac_critic_grad<ALGO>(__func__, env_kind, device, stream, obs_dev, action_dev, n_rows, idx_dev, batch, critic_dev, y_dev, grad_dev, stats_dev, workspace_dev,       \
                                 workspace_bytes, &pop);                                                                                                                        \
  }                                                                                                                                                                             \
  int PREFIX##actor_grad_members(int env_kind, int device, void* stream, int batch, int n_members, const float* actor_dev, size_t actor_stride_floats,                         \
                                 const float* critic_dev, size_t critic_stride_floats, const float* log_ent_coef_dev, const float* eps_dev, size_t eps_stride_floats,           \
                                 float* actor_grad_dev, float* ent_grad_dev, double* stats_dev, void* workspace_dev, size_t workspace_bytes) {                                  \
    const SacPop pop = {n_members, 0, actor_stride_floats, critic_stride_floats, eps_stride_floats, 0, 0, 0, nullptr};                                                          \
    return sac_actor_grad<ALGO>(__func__, env_kind, device, stream, batch, actor_dev, critic_dev, log_ent_coef_dev, eps_dev, actor_grad_dev, ent_grad_dev, stats_dev,          \
                                workspace_dev, workspace_bytes, &pop);                                                                                                          \
  }
TB_SAC_MEMBERS_ENTRIES(tb_sac_, SacAlgo)
TB_SAC_MEMBERS_ENTRIES(tb_tqc_, TqcAlgo)
#undef TB_SAC_MEMBERS_ENTRIES

int tb_sac_adam_members(int device, void* stream, float* params_dev, const float* grad_dev, float* exp_avg_dev, float* exp_avg_sq_dev, long long n, size_t stride_floats,
                        int n_members, const TbSacMemberHp* hp_dev, int which_lr, float beta1, float beta2, float eps, long long step, float* target_dev) {
  const char* who = "tb_sac_adam_members";
  if (n_members < 1 || n_members > TB_SAC_MAX_MEMBERS) return refusal(TB_E_INVAL, who, ": n_members must be in [1, 32767]");
  if (!params_dev || !hp_dev) return refusal(TB_E_INVAL, who, ": null argument");
  const bool polyak_only = !grad_dev && !exp_avg_dev && !exp_avg_sq_dev;
  if (polyak_only && !target_dev) return refusal(TB_E_INVAL, who, ": null argument (neither a gradient with both moments nor a target)");
  if (!polyak_only && (!grad_dev || !exp_avg_dev || !exp_avg_sq_dev)) return refusal(TB_E_INVAL, who, ": null argument (the gradient and both moments go together)");
  if (n < 1) return refusal(TB_E_INVAL, who, ": n must be >= 1");
  if (!polyak_only && step < 1) return refusal(TB_E_INVAL, who, ": step must be >= 1");
  if (which_lr != TB_SAC_LR_ACTOR && which_lr != TB_SAC_LR_CRITIC && which_lr != TB_SAC_LR_ENT) return refusal(TB_E_INVAL, who, ": which_lr must be a TB_SAC_LR_* name");
  if (misaligned(params_dev, 4) || misaligned(grad_dev, 4) || misaligned(exp_avg_dev, 4) || misaligned(exp_avg_sq_dev, 4) || misaligned(target_dev, 4) || misaligned(hp_dev, 8))
    return refusal(TB_E_INVAL, who, ": a float array is not 4-byte aligned, or hp not 8-byte aligned");
  if (stride_floats < (size_t)n) return refusal(TB_E_INVAL, who, ": stride_floats is shorter than n");
  if (!polyak_only && sac_rows_overlap(grad_dev, params_dev, stride_floats, n_members, n)) return refusal(TB_E_INVAL, who, ": the rows of grad_dev overlap the rows of params_dev");
  if (target_dev && sac_rows_overlap(target_dev, params_dev, stride_floats, n_members, n)) return refusal(TB_E_INVAL, who, ": the rows of target_dev overlap the rows of params_dev");
  DeviceGuard g;
  if (int rc = learner_device(g, device, who)) return rc;
  const SacAdamMembers mb = {(long long)stride_floats, hp_dev, which_lr};
  const dim3 grid(sac_blocks(n, 256), (unsigned)n_members);
  if (polyak_only) return launch(sac_polyak_kernel<SacAdamMembers>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)params_dev, target_dev, n, 0.0f, 0.0f, mb);
  const float c1 = (float)(1.0 - pow((double)beta1, (double)step)), c2 = (float)(1.0 - pow((double)beta2, (double)step));
  return launch(sac_adam_kernel<SacAdamMembers>, grid, dim3(256), 0, (hipStream_t)stream, params_dev, grad_dev, exp_avg_dev, exp_avg_sq_dev, n, 0.0f, beta1, beta2, eps, c1,
                c2, target_dev, 0.0f, 0.0f, mb);
}

int tb_sac_adam(int device, void* stream, float* params_dev, const float* grad_dev, float* exp_avg_dev, float* exp_avg_sq_dev, long long n, float lr, float beta1, float beta2,
                float eps, long long step, float* target_dev, float tau) {
  if (!params_dev) return fail(TB_E_INVAL, "tb_sac_adam: null argument (params)");
  if (n < 1) return fail(TB_E_INVAL, "tb_sac_adam: n must be >= 1");
  const bool polyak_only = !grad_dev && !exp_avg_dev && !exp_avg_sq_dev;
  if (polyak_only && !target_dev) return fail(TB_E_INVAL, "tb_sac_adam: null argument (neither a gradient with both moments nor a target)");
  if (!polyak_only && (!grad_dev || !exp_avg_dev || !exp_avg_sq_dev)) return fail(TB_E_INVAL, "tb_sac_adam: null argument (the gradient and both moments go together)");
  if (!polyak_only && step < 1) return fail(TB_E_INVAL, "tb_sac_adam: step must be >= 1");
  if (misaligned(params_dev, 4) || misaligned(grad_dev, 4) || misaligned(exp_avg_dev, 4) || misaligned(exp_avg_sq_dev, 4) || misaligned(target_dev, 4))
    return fail(TB_E_INVAL, "tb_sac_adam: a float array is not 4-byte aligned");
  if (target_dev == params_dev) return fail(TB_E_INVAL, "tb_sac_adam: target_dev must not be params_dev");
  DeviceGuard g;
  if (int rc = learner_device(g, device, "tb_sac_adam")) return rc;
  hipStream_t s = (hipStream_t)stream;
  const float omt = (float)(1.0 - (double)tau);
  const dim3 grid(sac_blocks(n, 256));
  if (polyak_only) return launch(sac_polyak_kernel<>, grid, dim3(256), 0, s, (const float*)params_dev, target_dev, n, omt, tau);
  const float c1 = (float)(1.0 - pow((double)beta1, (double)step)), c2 = (float)(1.0 - pow((double)beta2, (double)step));
  return launch(sac_adam_kernel<>, grid, dim3(256), 0, s, params_dev, grad_dev, exp_avg_dev, exp_avg_sq_dev, n, lr, beta1, beta2, eps, c1, c2, target_dev, omt, tau);
}

int tb_rollout(TbHandle* h, int n_steps, const float* actions_dev, float* obs_dev, float* reward_dev, uint8_t* done_dev,
               int32_t* substeps_total_dev, void* stream) {
  if (!h || !actions_dev || !obs_dev || !reward_dev || !done_dev) return fail(TB_E_INVAL, "tb_rollout: null argument");
  if (n_steps < 1) return fail(TB_E_INVAL, "tb_rollout: n_steps must be >= 1");
  if (!(h->kp.flags & TB_F_AUTO_RESET)) return fail(TB_E_UNSUPPORTED, "tb_rollout needs TB_F_AUTO_RESET (episodes must restart inside the launch)");
  DeviceGuard g(h->device);
  hipStream_t s = (hipStream_t)stream;
  if (h->pipeline && h->kind == TB_ENV_SWING && h->phase.valid && !substeps_total_dev) {
    // pipelined: launches that end where the episodes end, every one followed by its
    // fast-forward on a side stream instead of stalling its waves on it
    const size_t n = (size_t)h->n;
    for (int t = 0; t < n_steps;) {
      const int chunk = h->phase.chunk(n_steps - t);
      if (int rc = launch_step(h, chunk, actions_dev + (size_t)t * n * TB_SWING_ACT_DIM, obs_dev + (size_t)t * n * TB_SWING_OBS_DIM, reward_dev + (size_t)t * n,
                               done_dev + (size_t)t * n, nullptr, nullptr, s, nullptr, chunk > 1))
        return rc;
      t += chunk;
    }
    return TB_OK;
  }
  return launch_step(h, n_steps, actions_dev, obs_dev, reward_dev, done_dev, nullptr, substeps_total_dev, s);
}

int tb_get_state(TbHandle* h, uint32_t* words, uint8_t* done, int on_device, void* stream) {
  if (!h || !words) return fail(TB_E_INVAL, "tb_get_state: null argument");
  DeviceGuard g(h->device);
  hipStream_t s = (hipStream_t)stream;
  if (int rc = flush_all(h, s)) return rc;
  const size_t wb = sizeof(uint32_t) * (size_t)words_of(h->kind) * h->n;
  hipMemcpyKind k = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  HIP_TRY(hipMemcpyAsync(words, h->d_words, wb, k, s));
  if (done) HIP_TRY(hipMemcpyAsync(done, h->d_done, (size_t)h->n, k, s));
  if (!on_device) HIP_TRY(hipStreamSynchronize(s));
  return TB_OK;
}

int tb_set_state(TbHandle* h, const uint32_t* words, const uint8_t* done, int on_device, void* stream) {
  if (!h || !words) return fail(TB_E_INVAL, "tb_set_state: null argument");
  DeviceGuard g(h->device);
  hipStream_t s = (hipStream_t)stream;
  if (int rc = flush_all(h, s)) return rc;
  h->phase.invalidate();  // injected states need not be in lockstep
  const size_t wb = sizeof(uint32_t) * (size_t)words_of(h->kind) * h->n;
  hipMemcpyKind k = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  HIP_TRY(hipMemcpyAsync(h->d_words, words, wb, k, s));
  if (done) HIP_TRY(hipMemcpyAsync(h->d_done, done, (size_t)h->n, k, s));
  else HIP_TRY(hipMemsetAsync(h->d_done, 0, (size_t)h->n, s));
  HIP_TRY(hipMemsetAsync(h->d_mflag, 0, (size_t)h->n, s));  // the racket<->court contact caches are not part of the state words
  if (h->kind == TB_ENV_SWING && h->pipeline) { if (int rc = rederive_phase(h, s)) return rc; }
  if (!on_device) HIP_TRY(hipStreamSynchronize(s));
  return TB_OK;
}

int tb_counters(TbHandle* h, uint64_t* out, void* stream) {
  if (!h || !out) return fail(TB_E_INVAL, "tb_counters: null argument");
  DeviceGuard g(h->device);
  static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "counter width");
  uint64_t shards[TB_COUNTER_SHARDS][TB_N_COUNTERS];
  if (int rc = read_back(h, shards, h->d_counters, sizeof shards, (hipStream_t)stream)) return rc;
  for (int k = 0; k < TB_N_COUNTERS; ++k) {
    out[k] = 0;
    for (int sh = 0; sh < TB_COUNTER_SHARDS; ++sh) out[k] += shards[sh][k];
  }
  out[6] += h->first_substeps;
  return TB_OK;
}

int tb_sealed_substeps(TbHandle* h, uint64_t* out, void* stream) {
  if (!h || !out) return fail(TB_E_INVAL, "tb_sealed_substeps: null argument");
  DeviceGuard g(h->device);
  return read_back(h, out, h->d_counters + kSealedWord, sizeof(uint64_t), (hipStream_t)stream);
}

int tb_diag_stream_copy(const uint32_t* src_dev, uint32_t* dst_dev, int n, int rows, int device, void* stream) {
  if (!src_dev || !dst_dev || n <= 0 || rows <= 0) return fail(TB_E_INVAL, "tb_diag_stream_copy: bad argument");
  DeviceGuard g(device);
  if (g.err != hipSuccess) return fail((int)g.err, "hipSetDevice");
  hipLaunchKernelGGL(tb_diag_copy_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src_dev, dst_dev, n, rows);
  HIP_TRY(hipGetLastError());
  return TB_OK;
}

// ------------------------------------------------------------------------------------------ tb_render (csrc/tb_render.hpp)
int tb_render(int env_kind, int device, void* stream, const TbParams* params, const uint32_t* words_dev, int n_envs, const int32_t* env_idx_dev_or_null,
              int n_images, const TbCamera* camera, int width, int height, uint8_t* rgb_dev, uint8_t* id_dev_or_null, float* depth_dev_or_null) {
  if (!kind_ok(env_kind)) return fail(TB_E_INVAL, "tb_render: unknown env kind");
  if (!params || !words_dev || !camera || !rgb_dev) return fail(TB_E_INVAL, "tb_render: null argument (params, words, camera and rgb are required)");
  if (params->n_hull < 3 || params->n_hull > TB_MAX_HULL) return fail(TB_E_INVAL, "tb_render: TbParams.n_hull must be in [3, 64]");
  if (n_envs < 1 || n_images < 1 || width < 1 || height < 1) return fail(TB_E_INVAL, "tb_render: n_envs, n_images, width and height must be >= 1");
  if (width > 16384 || height > 16384) return fail(TB_E_INVAL, "tb_render: width and height must be <= 16384");
  if (!env_idx_dev_or_null && n_images > n_envs) return fail(TB_E_INVAL, "tb_render: without env_idx image k shows env k: n_images must be <= n_envs");
  if (camera->struct_size != sizeof(TbCamera)) return fail(TB_E_INVAL, "tb_render: TbCamera.struct_size is not sizeof(TbCamera)");
  if (misaligned(words_dev, 4) || misaligned(env_idx_dev_or_null, 4) || misaligned(depth_dev_or_null, 4)) return fail(TB_E_INVAL, "tb_render: words, env_idx and depth must be 4-byte aligned");
  const int tiles_x = (width + 7) / 8, tiles = tiles_x * ((height + 7) / 8);
  if ((long long)tiles * n_images > 0x7fffffffLL) return fail(TB_E_INVAL, "tb_render: more than 2^31 - 1 tiles in one call");
  // the camera basis, float64 (tb_render.hpp, THE RULE)
  RenderCam cam;
  double f[3], r[3], u[3], l[3], fl = 0.0, ul = 0.0, ll = 0.0, rl = 0.0;
  for (int i = 0; i < 3; ++i) {
    if (!isfinite(camera->eye[i]) || !isfinite(camera->target[i]) || !isfinite(camera->up[i]) || !isfinite(camera->light_dir[i]))
      return fail(TB_E_INVAL, "tb_render: a camera vector is not finite");
    f[i] = (double)camera->target[i] - (double)camera->eye[i];
    fl += f[i] * f[i]; ul += (double)camera->up[i] * camera->up[i]; ll += (double)camera->light_dir[i] * camera->light_dir[i];
  }
  if (!(fl > 0.0)) return fail(TB_E_INVAL, "tb_render: eye == target");
  if (!(ul > 0.0)) return fail(TB_E_INVAL, "tb_render: up is the zero vector");
  if (!(ll > 0.0)) return fail(TB_E_INVAL, "tb_render: light_dir is the zero vector");
  if (!(camera->fov_y_deg > 0.0f && camera->fov_y_deg < 180.0f)) return fail(TB_E_INVAL, "tb_render: fov_y_deg must be in (0, 180)");
  if (camera->follow != 0 && camera->follow != 1) return fail(TB_E_INVAL, "tb_render: follow must be 0 or 1");
  fl = sqrt(fl);
  for (int i = 0; i < 3; ++i) f[i] /= fl;
  r[0] = f[1] * camera->up[2] - f[2] * camera->up[1]; r[1] = f[2] * camera->up[0] - f[0] * camera->up[2]; r[2] = f[0] * camera->up[1] - f[1] * camera->up[0];
  for (int i = 0; i < 3; ++i) rl += r[i] * r[i];
  if (!(rl > 1e-12 * ul)) return fail(TB_E_INVAL, "tb_render: up is parallel to the view direction");
  rl = sqrt(rl);
  for (int i = 0; i < 3; ++i) r[i] /= rl;
  u[0] = r[1] * f[2] - r[2] * f[1]; u[1] = r[2] * f[0] - r[0] * f[2]; u[2] = r[0] * f[1] - r[1] * f[0];
  const double th = tan(0.5 * (double)camera->fov_y_deg * 3.14159265358979323846 / 180.0), tw = th * (double)width / (double)height;
  ll = sqrt(ll);
  for (int i = 0; i < 3; ++i) {
    l[i] = camera->light_dir[i] / ll;
    cam.eye[i] = camera->eye[i]; cam.fwd[i] = (float)f[i]; cam.right[i] = (float)(tw * r[i]); cam.up[i] = (float)(th * u[i]); cam.light[i] = (float)l[i];
  }
  cam.follow = camera->follow;
  RenderScene sc;
  for (int i = 0; i < 3; ++i) { sc.ground_half[i] = params->ground_half[i]; sc.net_half[i] = params->net_half[i]; }
  sc.goal_radius = params->goal_radius; sc.goal_half_len = params->goal_half_len; sc.ball_radius = params->ball_radius;
  sc.half_thick = params->racket_half_thick; sc.bound_radius = params->hull_bound_radius; sc.racket_scale = params->racket_scale;
  sc.n_hull = params->n_hull; sc.flags = params->flags;
  RenderHull hull;
  for (int i = 0; i < TB_MAX_HULL; ++i) {
    const bool in = i < params->n_hull;
    hull.e[i] = make_float4(in ? params->hull_edges[i][0] : 0.0f, in ? params->hull_edges[i][1] : 0.0f, in ? params->hull_edges[i][2] : 0.0f, in ? params->hull_edges[i][3] : 0.0f);
  }
  DeviceGuard g;
  if (int rc = learner_device(g, device, "tb_render")) return rc;
  const dim3 grid((unsigned)(tiles * n_images)), block(64);
  if (env_kind == TB_ENV_SWING)
    return launch(tb_render_kernel<TB_ENV_SWING>, grid, block, 0, (hipStream_t)stream, cam, sc, hull, words_dev, n_envs, env_idx_dev_or_null, width, height, tiles_x, tiles,
                  rgb_dev, id_dev_or_null, depth_dev_or_null);
  return launch(tb_render_kernel<TB_ENV_TENNIS>, grid, block, 0, (hipStream_t)stream, cam, sc, hull, words_dev, n_envs, env_idx_dev_or_null, width, height, tiles_x, tiles,
                rgb_dev, id_dev_or_null, depth_dev_or_null);
}

// ------------------------------------------------------------------------------------------ tb_swing_trace (csrc/tb_trace.hpp)
int tb_swing_trace(TbHandle* h, const uint32_t* words_dev, const uint8_t* done_dev, int n_rows, const float* actions_dev, int stride, int max_frames,
                   uint32_t* frames_dev, int32_t* n_frames_dev, float* reward_dev, int32_t* substeps_dev, uint8_t* done_out_dev, float* obs_dev_or_null,
                   void* stream) {
  if (!h) return fail(TB_E_INVAL, "tb_swing_trace: null handle");
  if (!words_dev || !done_dev || !actions_dev || !frames_dev || !n_frames_dev || !reward_dev || !substeps_dev || !done_out_dev)
    return fail(TB_E_INVAL, "tb_swing_trace: null argument (only obs may be null)");
  if (h->kind != TB_ENV_SWING) return fail(TB_E_INVAL, "tb_swing_trace: a SwingRacket-v0 handle is required (every Tennisbot-v0 agent step is one substep, visible as it is)");
  if (n_rows < 1 || stride < 1 || max_frames < 1) return fail(TB_E_INVAL, "tb_swing_trace: n_rows, stride and max_frames must be >= 1");
  if (n_rows > (1 << 25)) return fail(TB_E_INVAL, "tb_swing_trace: n_rows must be <= 2^25");  // (32-bit row offsets inside a frame: see row_word)
  if (misaligned(words_dev, 4) || misaligned(frames_dev, 4) || misaligned(n_frames_dev, 4) || misaligned(reward_dev, 4) || misaligned(substeps_dev, 4))
    return fail(TB_E_INVAL, "tb_swing_trace: words, frames, n_frames, reward and substeps must be 4-byte aligned");
  if (misaligned(actions_dev, 8) || misaligned(obs_dev_or_null, 8)) return fail(TB_E_INVAL, "tb_swing_trace: actions and obs must be 8-byte aligned (rows are accessed two floats at a time)");
  DeviceGuard g(h->device);
  if (g.err != hipSuccess) return fail((int)g.err, "hipSetDevice");
  TraceArgs a;
  memset(&a, 0, sizeof a);
  a.P = h->kp; a.hull = h->d_hull;
  a.words = words_dev; a.done = done_dev; a.actions = actions_dev;
  a.frames = frames_dev; a.n_frames = n_frames_dev; a.reward = reward_dev; a.substeps = substeps_dev; a.done_out = done_out_dev; a.obs = obs_dev_or_null;
  a.n = n_rows; a.stride = stride; a.max_frames = max_frames;
  const bool rg = extended_contacts(h->kp);
  const dim3 grid((unsigned)((n_rows + 63) / 64));
  return launch(rg ? tb_swing_trace_kernel<true> : tb_swing_trace_kernel<false>, grid, dim3(64), dyn_lds(ff_lds_words(rg, false), 64), (hipStream_t)stream, a);
}

int tb_diag_two_wave_gate(TbHandle* h, uint8_t* out_dev, void* stream) {
  if (!h || !out_dev || h->kind != TB_ENV_SWING) return fail(TB_E_INVAL, "tb_diag_two_wave_gate: bad argument");
  DeviceGuard g(h->device);
  if (int rc = flush_all(h, (hipStream_t)stream)) return rc;
  hipLaunchKernelGGL(tb_diag_two_wave_gate_kernel, dim3((unsigned)((h->n + 63) / 64)), dim3(64), 0, (hipStream_t)stream, base_args(h), out_dev);
  HIP_TRY(hipGetLastError());
  return TB_OK;
}

int tb_diag_idle(int waves, int microseconds, int device, void* stream) {
  if (waves <= 0 || microseconds <= 0) return fail(TB_E_INVAL, "tb_diag_idle: bad argument");
  DeviceGuard g(device);
  if (g.err != hipSuccess) return fail((int)g.err, "hipSetDevice");
  hipLaunchKernelGGL(tb_diag_idle_kernel, dim3((unsigned)waves), dim3(64), 0, (hipStream_t)stream, (unsigned long long)microseconds * 100ull);
  HIP_TRY(hipGetLastError());
  return TB_OK;
}

// (diagnostic builds only: tb_diag_read_stamps / tb_diag_read_lanes)
#define TB_DIAG_HOST_SECTION
#include "tb_diag.hpp"
#undef TB_DIAG_HOST_SECTION

int tb_counters_reset(TbHandle* h, void* stream) {
  if (!h) return fail(TB_E_INVAL, "tb_counters_reset: null handle");
  DeviceGuard g(h->device);
  HIP_TRY(hipMemsetAsync(h->d_counters, 0, sizeof(uint64_t) * kCounterWords, (hipStream_t)stream));
  h->first_substeps = 0;
  return TB_OK;
}

}  // extern "C"

// tb_trace.hpp -- the flight of a SwingRacket-v0 ball, substep by substep: tb_swing_trace runs ONE agent step of caller-owned states
// and stores the states it passes through. Additive: it reads state words, the handle's parameter block and outline table, and writes
// caller-owned buffers; no step / fast-forward / pool kernel knows of it. Included by tb_stepper.hip after tb_kernels.hpp.
//
// A SwingRacket-v0 episode is 25 swing steps and one last step whose fast-forward (swingracket_env.py:105-141) runs up to 775 more
// physics substeps inside env.step(): whether the ball reaches the goal, where it lands, whether the racket clips it again all happen
// there, and tb_step shows only the reward, the terminal observation and a substep count.
//
// WHICH SUBSTEPS BECOME FRAMES (include/tb_stepper.h states the same rule; stepper.trace_frame_substeps is it in plain Python)
// Number the substeps of the call s = 1 .. ns: s = 1 is the agent's substep, ns what tb_step reports in substeps_dev (1 .. 776). The
// sampled set is {1 + j stride : j >= 0, 1 + j stride <= ns} plus ns itself, in increasing order: m = 1 + (ns - 1) / stride +
// ((ns - 1) % stride != 0) samples.
//   m <= max_frames: row k < m holds the state after the k-th sampled substep, rows m .. max_frames - 1 copies of the final state (a
//                    tiled film of envs with different flight lengths shows the landed ball; no byte of the buffer stays unwritten);
//   m >  max_frames: rows 0 .. max_frames - 2 hold the first max_frames - 1 samples, row max_frames - 1 the state after substep ns.
// The last stored row is always the final state, and n_frames[i] = m in both cases (as snprintf reports the length it needed). A
// row's step-count word is the input step count + s, the episode word is the input's: the trace never resets an env, whatever
// TB_F_AUTO_RESET says.
//
// WHY A CUT FLIGHT IS THE UNCUT FLIGHT, BIT FOR BIT. The loop's whole state between two substeps is the env's registers, the
// racket<->court cache and the force the next substep starts with -- and that force is a function of the registers
// (restoring_force(e), swingracket_env.py:135-141; none before the first flight substep: the agent's substep cleared the
// accumulators). swing_loop<FORM, BUDGET = true> leaves after `budget` substeps with exactly that state, and the next call recomputes
// the force from it with the same operations: what the phased fast-forward (tb_ff_kernel) relies on, here with budget = stride and
// the lane keeping its registers and its LDS column instead of travelling through a parked record.
//
// Shape: one lane per traced env, one-wave workgroups, tb_ff_kernel<RG, false>'s form of the substep -- FORM = SF_RG | SF_REGGROUND
// with the extended contact set, else 0: nothing in it assumes a full wave or skips a substep, since lanes here finish at different
// substeps and non-flight rows (one substep, one frame) share waves with flights. The agent's substep is swing_step's with defer =
// true (a pending restoring force, TB_DONE_PENDING_FORCE, included); a lane it parked then repeats the budgeted loop until its env is
// done, while any lane of the wave is unfinished. Frames are [row][word][lane]: frames + row * words * n is a words_dev for tb_render,
// and the 64 lanes of a wave store 64 consecutive words per state word -- plain vector stores. Counters are the handle's, and the trace
// does not touch the handle: the events of a traced step are counted nowhere.
#pragma once

namespace {

struct TraceArgs {
  KParams P;
  const float4* hull;      // the handle's outline table, staged into LDS
  const uint32_t* words;   // [TB_SWING_WORDS][n] tb_get_state's layout
  const uint8_t* done;     // [n]
  const float* actions;    // [n][6]
  uint32_t* frames;        // [max_frames][TB_SWING_WORDS][n]
  int32_t* n_frames;       // [n]
  float* reward;           // [n]
  int32_t* substeps;       // [n]
  uint8_t* done_out;       // [n]
  float* obs;              // [n][6] or null
  int n, stride, max_frames;
};

// the state row of lane i as tb_get_state gives it, into the frame that starts at `w`
TB_DEV void store_frame(uint32_t* w, int n, int i, const EnvRegs& e) {
  constexpr int K = TB_ENV_SWING;
  st<K>(w, TB_W_RP, n, i, e.r.p.x); st<K>(w, TB_W_RP + 1, n, i, e.r.p.y); st<K>(w, TB_W_RP + 2, n, i, e.r.p.z);
  st<K>(w, TB_W_RQ, n, i, e.r.q.x); st<K>(w, TB_W_RQ + 1, n, i, e.r.q.y); st<K>(w, TB_W_RQ + 2, n, i, e.r.q.z); st<K>(w, TB_W_RQ + 3, n, i, e.r.q.w);
  st<K>(w, TB_W_RV, n, i, e.r.v.x); st<K>(w, TB_W_RV + 1, n, i, e.r.v.y); st<K>(w, TB_W_RV + 2, n, i, e.r.v.z);
  st<K>(w, TB_W_RW, n, i, e.r.w.x); st<K>(w, TB_W_RW + 1, n, i, e.r.w.y); st<K>(w, TB_W_RW + 2, n, i, e.r.w.z);
  st<K>(w, TB_W_BP, n, i, e.b.p.x); st<K>(w, TB_W_BP + 1, n, i, e.b.p.y); st<K>(w, TB_W_BP + 2, n, i, e.b.p.z);
  st<K>(w, TB_W_BV, n, i, e.b.v.x); st<K>(w, TB_W_BV + 1, n, i, e.b.v.y); st<K>(w, TB_W_BV + 2, n, i, e.b.v.z);
  st<K>(w, TB_W_BW, n, i, e.b.w.x); st<K>(w, TB_W_BW + 1, n, i, e.b.w.y); st<K>(w, TB_W_BW + 2, n, i, e.b.w.z);
#pragma unroll
  for (int k = 0; k < 6; ++k) st<K>(w, TB_W_SW_GOAL + k, n, i, e.aux[k]);
  row_store<true>(w, TB_W_SW_STEP, n, i, (uint32_t)e.step_count);
  row_store<true>(w, TB_W_SW_EPISODE, n, i, e.episode);
}

template <bool RG>
__global__ void __launch_bounds__(64, 1) tb_swing_trace_kernel(TraceArgs A) {
  constexpr unsigned FORM = RG ? (SF_RG | SF_REGGROUND) : 0u;  // the small-batch fast-forward's
  __shared__ float4 s_hull[TB_HULL_LDS];
  const int lane = threadIdx.x & 63;
  stage_hull(s_hull, A.hull, A.P.n_hull);
  __syncthreads();
  const int i = blockIdx.x * 64 + lane;
  const bool live = i < A.n;
  const size_t frame_words = (size_t)TB_SWING_WORDS * (size_t)A.n;
  const vec3 zero = mk(0.0f, 0.0f, 0.0f);
  uint32_t cnt[TB_N_COUNTERS] = {};  // (what the substeps count; dropped: the handle's counters are not the trace's to touch)
  TB_DIAG_STAMPS_BEGIN(st);
  EnvRegs e;
  Manifold M;
  init_manifold(M, lane, 64, true);  // an empty racket<->court cache, as a restored state starts with
  bool flying = false;
  int ns = 0, k = 0, m = 0;  // substeps so far; the next row to store; samples so far
  float rew = 0.0f;
  if (live) {
    float a[TB_SWING_ACT_DIM];
    load_env<TB_ENV_SWING>(A.words, A.done, A.n, i, e);
    load_actions<TB_ENV_SWING>(A.actions, (size_t)i, a);
    rew = swing_step<FORM>(A.P, s_hull, e, M, a, ns, cnt, true, flying TB_STAMP_PASS);  // s = 1
    m = 1;
    if (flying && k < A.max_frames - 1) { store_frame(A.frames + (size_t)k * frame_words, A.n, i, e); ++k; }
  }
  bool first = true;  // the first flight substep runs with no force at all, every later one with the restoring force of the state before it
  while (__any(flying)) {
    if (flying) {
      flying = false;
      rew = swing_loop<FORM, true>(A.P, s_hull, e, M, first ? zero : restoring_force(e), zero, true, false, flying, ns, cnt TB_STAMP_PASS, A.stride);
      ++m;  // s = 1 + j stride (still flying), or ns
      if (flying && k < A.max_frames - 1) { store_frame(A.frames + (size_t)k * frame_words, A.n, i, e); ++k; }
    }
    first = false;
  }
  // the final state into row k and every row behind it, the wave's lanes side by side row by row
  int k_min = live ? k : A.max_frames;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { const int o = __shfl_xor(k_min, off, 64); k_min = o < k_min ? o : k_min; }
  for (int r = k_min; r < A.max_frames; ++r)
    if (live && r >= k) store_frame(A.frames + (size_t)r * frame_words, A.n, i, e);
  if (live) {
    A.n_frames[i] = m;
    A.reward[i] = rew;  // (every reward of the flight is paid in its last substep; a non-flight row's is the agent substep's contact bonus)
    A.substeps[i] = ns;
    A.done_out[i] = e.done != TB_DONE_NO ? 1 : 0;
    if (A.obs) {
      float o[TB_SWING_OBS_DIM];
      make_obs<TB_ENV_SWING>(e, o);
      write_obs<TB_ENV_SWING>(A.obs, (size_t)i, o);
    }
  }
}

}  // namespace

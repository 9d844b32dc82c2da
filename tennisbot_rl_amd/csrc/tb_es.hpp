// Evolution-strategies population evaluation (tb_es_evaluate): one lane per env runs a whole episode with its member's GatedCNN
// inside the step loop. Device code only; included by tb_stepper.hip after tb_kernels.hpp (KArgs, EnvRegs, swing_step,
// tennis_step, end_agent_step, flush_counters, fast_tanh are defined there). Part of the library's single translation unit.
//
// What one lane computes is the reference's fitness_static (tennisbot/ES/fitness_functions.py:17-159) for one episode:
//   * a FRESH Normalizer(O) per episode (evolution_strategy_static.py:25-44; the pool pickles the generation's zero normaliser
//     into every worker, :166, :265), float64, elementwise, in the reference's statement order:
//       n += 1; last = mean; mean += (x - mean) / n; mean_diff += (x - last) * (x - mean); var = clip(mean_diff / n, min=1e-2)
//       normalize(x) = (x - mean) / sqrt(var), rounded to float32 (torch.from_numpy(x).float())
//     true IEEE division and square root (hipcc's default for double), no contraction (-ffp-contract=off); np.clip keeps NaN.
//     The normaliser lives in REGISTERS (2 O + 1 doubles: 26 / 50 VGPRs): it is read and written in full every step, and the
//     substep, which needs the register file most, runs between two uses, where the compiler may keep it or not as it likes.
//   * the history: 8 x normalize(obs0), then one normalised row appended per step, older rows never renormalised;
//   * GatedCNN(O, A) (tennisbot/ES/policies.py:59-130) on the last 8 rows:
//       h0 = tanh(conv_0(x)) * sigmoid(conv_gate_0(x))    8 channels, kernel 2, dilation 1   (8 -> 7 columns)
//       h1 = tanh(conv_1(h0)) * sigmoid(conv_gate_1(h0))  12 channels, kernel 2, dilation 2  (7 -> 5)
//       out = conv_2(h1)                                   A channels, kernel 2, dilation 4   (5 -> 1)
//     a = clip(out, -1, 1), NaN kept (clip_action);
//   * rew_ep += reward in float64, in step order, until done.
//
// STREAMING. The window slides by one row per step, and every column of every layer depends only on its own inputs: the last
// h0 column is f(x[t-1], x[t]), the last h1 column g(h0[t-2], h0[t]), the output c(h1[t-4], h1[t]). Each step therefore
// computes ONE new h0 column, ONE new h1 column and the output -- the same operations on the same inputs as recomputing the
// window, ~800 FMAs instead of ~4600. Rows before the episode's first are copies of x0, so at step 0 every column of a layer is
// the same value, computed once from (x0, x0) and written to every ring slot. Rings of 3 h0 and 5 h1 columns and x[t-1] live in
// the lane's LDS column (90 / 96 words per lane, [word][64 lanes]: no bank conflicts, slot indices need no register arrays).
//
// ARITHMETIC: float32, explicit fmaf. A column's pre-activation is bias, then for every input channel in order tap 0 (the
// earlier column) and tap 1 (the later), one fmaf each. tanh on the exp2 / rcp units (fast_tanh, tb_policy.hpp: absolute error
// < 3e-7); sigmoid(z) = 1 / (1 + 2^(-z log2 e)) on the same units: the exp2 and the reciprocal are within 1 ulp, the scaling
// of z rounds by 2^-24 relative, and the result's sensitivity to a relative error r of the exponential is s (1 - s) r with
// s (1 - s) |z| <= 0.224: absolute error < 3e-7 (stated as ES_SIGMOID_ERR in tests/es_reference.py). Both saturate exactly
// at +-inf and keep NaN.
//
// WEIGHTS: member m's parameter vector is row m of weights (nn.utils.parameters_to_vector order, es_floats); env i uses member
// i / envs_per_member. A wave whose 64 envs span at most TB_ES_LDS_MEMBERS members (the reference's 10 episodes per member: at
// most 8) stages those rows in LDS first; otherwise (envs_per_member = 1: 64 members) every lane reads its row from global memory.
//
// ENV STEP: tennis_step / swing_step exactly as the other kernels call them. SwingRacket episodes are exactly 26 agent steps and
// the 26th always starts the fast-forward: that lane is PARKED (park_for_ff) and tb_ff_kernel finishes it; the host folds the
// terminal reward into the return after the pipeline's flush (tb_es_fold_kernel). Lanes whose episode is over -- and lanes beyond
// n -- step the idle dummy (idle_env) so that every lane stays in the shared substep; a wave runs until its last lane is done.
#pragma once

namespace {

// GatedCNN parameter layout (parameters_to_vector order): conv_0.w [8][O][2], conv_0.b [8], conv_gate_0.w/b, conv_1.w [12][8][2],
// conv_1.b [12], conv_gate_1.w/b, conv_2.w [A][12][2], conv_2.b [A]
template <int KIND> struct EsNet {
  static constexpr int O = Dims<KIND>::O, A = Dims<KIND>::A, C0 = 8, C1 = 12;
  static constexpr int W0 = 0, B0 = W0 + C0 * O * 2, G0W = B0 + C0, G0B = G0W + C0 * O * 2;
  static constexpr int W1 = G0B + C0, B1 = W1 + C1 * C0 * 2, G1W = B1 + C1, G1B = G1W + C1 * C0 * 2;
  static constexpr int W2 = G1B + C1, B2 = W2 + A * C1 * 2, P = B2 + A;
  static constexpr int PP = (P + 3) / 4 * 4;  // a staged row, padded to whole float4s
  // LDS ring words per lane: x[t-1], 3 h0 columns, 5 h1 columns
  static constexpr int R_X = 0, R_H0 = O, R_H1 = O + 3 * C0, RING = O + 3 * C0 + 5 * C1;
};
template <int KIND> constexpr int es_floats() { return EsNet<KIND>::P; }
static_assert(EsNet<TB_ENV_SWING>::P == 766 && EsNet<TB_ENV_TENNIS>::P == 858, "GatedCNN parameter counts of the reference");
constexpr int TB_ES_LDS_MEMBERS = 8;

// the static contact rows: registers for Tennisbot without the extended contact set, the lane's LDS column otherwise -- the split of
// the step kernels (step_rows_in_registers), whose results the evaluation reproduces (with RG, Tennisbot's register form stepped a
// ball-court bounce differently from tb_step in the replay test); dynamic LDS words per lane:
constexpr bool es_rows_in_registers(int kind, bool rg) { return kind == TB_ENV_TENNIS && !rg; }
constexpr int es_lds_words(int kind, bool rg) { return lds_words(!es_rows_in_registers(kind, rg), rg); }

struct EsArgs {
  const float* weights;  // [n_members][stride]
  size_t stride;         // floats between members' rows (multiple of 4, >= es_floats)
  int per_member;        // envs per member
  double* ret;           // [n] episode return (SwingRacket: without the terminal reward, which tb_es_fold_kernel adds)
  int32_t* len;          // [n] episode length in agent steps
  // optional trace, rows [t][n] (TbEsTrace); t_max = 0: off
  int t_max;
  float *t_net_in, *t_obs, *t_act, *t_raw, *t_rew;
  uint8_t* t_done;
};

// sigmoid on the exp2 / rcp units (error bound in the header comment)
TB_DEV float fast_sigmoid(float z) { return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(z * -1.4426950408889634f)); }

// one gated column: h[c] = tanh(bias + sum_k taps) * sigmoid(gate bias + sum_k gate taps), inputs a (tap 0) and b (tap 1) with
// element strides SA / SB (64: the lane's LDS column; 1: the caller's registers); out: the lane's LDS column
template <int CIN, int COUT, int SA, int SB>
TB_DEV void es_gated(const float* W, int w_off, int b_off, int g_off, int gb_off, const float* a, const float* b, float* out) {
#pragma unroll 2
  for (int c = 0; c < COUT; ++c) {
    float z = W[b_off + c], g = W[gb_off + c];
#pragma unroll
    for (int k = 0; k < CIN; ++k) {
      const float xa = a[k * SA], xb = b[k * SB];
      z = FMA(W[w_off + (c * CIN + k) * 2], xa, z);
      z = FMA(W[w_off + (c * CIN + k) * 2 + 1], xb, z);
      g = FMA(W[g_off + (c * CIN + k) * 2], xa, g);
      g = FMA(W[g_off + (c * CIN + k) * 2 + 1], xb, g);
    }
    out[c * 64] = fast_tanh(z) * fast_sigmoid(g);
  }
}

// the network's step t for one lane: x = the normalised row appended at step t; ring = the lane's LDS column (stride 64)
template <int KIND>
TB_DEV void es_net_step(const float* W, const float* x, float* ring, int t, float* raw) {
  using N = EsNet<KIND>;
  constexpr int L = 64;
  float* h0 = ring + N::R_H0 * L;
  float* h1 = ring + N::R_H1 * L;
  if (t == 0) {  // every column of the window is f(x0, x0): compute once, fill every slot
    es_gated<N::O, N::C0, 1, 1>(W, N::W0, N::B0, N::G0W, N::G0B, x, x, h0);
    es_gated<N::C0, N::C1, L, L>(W, N::W1, N::B1, N::G1W, N::G1B, h0, h0, h1);
#pragma unroll
    for (int c = 0; c < N::C0; ++c) { const float v = h0[c * L]; h0[(N::C0 + c) * L] = v; h0[(2 * N::C0 + c) * L] = v; }
#pragma unroll
    for (int c = 0; c < N::C1; ++c) {
      const float v = h1[c * L];
#pragma unroll
      for (int s = 1; s < 5; ++s) h1[(s * N::C1 + c) * L] = v;
    }
  } else {
    float* h0_new = h0 + (t % 3) * N::C0 * L;
    const float* h0_old = h0 + ((t + 1) % 3) * N::C0 * L;  // h0[t - 2]
    es_gated<N::O, N::C0, L, 1>(W, N::W0, N::B0, N::G0W, N::G0B, ring + N::R_X * L, x, h0_new);
    es_gated<N::C0, N::C1, L, L>(W, N::W1, N::B1, N::G1W, N::G1B, h0_old, h0_new, h1 + (t % 5) * N::C1 * L);
  }
  const float* h1_new = h1 + (t % 5) * N::C1 * L;
  const float* h1_old = h1 + ((t + 1) % 5) * N::C1 * L;  // h1[t - 4]
#pragma unroll
  for (int a = 0; a < N::A; ++a) {
    float z = W[N::B2 + a];
#pragma unroll
    for (int k = 0; k < N::C1; ++k) {
      z = FMA(W[N::W2 + (a * N::C1 + k) * 2], h1_old[k * L], z);
      z = FMA(W[N::W2 + (a * N::C1 + k) * 2 + 1], h1_new[k * L], z);
    }
    raw[a] = z;
  }
#pragma unroll
  for (int k = 0; k < N::O; ++k) ring[(N::R_X + k) * L] = x[k];  // x[t] is the next step's x[t-1]
}

// the float64 normaliser of one lane: observe(o), then the float32 rounding of normalize(o)
template <int NO>
TB_DEV void es_normalise(double& n, double* mean, double* mdiff, const float* o, float* x) {
  n += 1.0;
#pragma unroll
  for (int k = 0; k < NO; ++k) {
    const double v = (double)o[k], last = mean[k];
    mean[k] += (v - mean[k]) / n;
    mdiff[k] += (v - last) * (v - mean[k]);
    double var = mdiff[k] / n;
    var = var != var ? var : (var < 1e-2 ? 1e-2 : var);  // ndarray.clip(min=1e-2): NaN kept
    x[k] = (float)((v - mean[k]) / sqrt(var));
  }
}

template <int KIND, bool RG>
__global__ void __launch_bounds__(64) tb_es_rollout_kernel(KArgs A, EsArgs E) {
  using N = EsNet<KIND>;
  constexpr int NA = Dims<KIND>::A, NO = Dims<KIND>::O, T_MAX = episode_cap(KIND);
  __shared__ float4 s_hull[TB_HULL_LDS];
  __shared__ __attribute__((aligned(16))) float s_w[TB_ES_LDS_MEMBERS * N::PP];
  __shared__ float s_ring[N::RING * 64];
  const int lane = threadIdx.x, i = blockIdx.x * 64 + lane;
  const bool live = i < A.n;
  const int first = blockIdx.x * 64, last = min(first + 63, A.n - 1);
  const int m0 = first / E.per_member, nm = last / E.per_member - m0 + 1;
  const bool staged = nm <= TB_ES_LDS_MEMBERS;  // wave-uniform
  if (staged) {
    for (int k = lane; k < nm * (N::PP / 4); k += 64) {
      const int r = k / (N::PP / 4), c = k % (N::PP / 4);
      reinterpret_cast<float4*>(s_w)[k] = *reinterpret_cast<const float4*>(E.weights + (size_t)(m0 + r) * E.stride + 4 * c);
    }
  }
  stage_hull(s_hull, A.hull, A.P.n_hull);
  __syncthreads();  // (the staged rows too)
  const int m = (live ? i : last) / E.per_member;
  const float* W = staged ? s_w + (m - m0) * N::PP : E.weights + (size_t)m * E.stride;
  float* ring = s_ring + lane;

  EnvRegs e;
  Manifold M;
  enter_env_wave<KIND>(A, i, live, lane, !es_rows_in_registers(KIND, RG), e, M);  // the state tb_reset just wrote: the episode's start, no contacts cached
  uint32_t cnt[TB_N_COUNTERS] = {};
  KParams Pl = A.P;
  double nrm = 0.0, mean[NO], mdiff[NO];
#pragma unroll
  for (int k = 0; k < NO; ++k) { mean[k] = 0.0; mdiff[k] = 0.0; }
  float o[NO];
  make_obs<KIND>(e, o);
  EpisodeTally ep = {live, 0.0, 0};
  constexpr unsigned FORM = loop_step_form(RG, true, es_rows_in_registers(KIND, RG));
  TB_DIAG_STAMPS_BEGIN(st);  // (the substep's stamps: the diagnostic build compiles every kernel that steps envs)
  for (int t = 0; t < T_MAX && __ballot(ep.active) != 0ull; ++t) {
    float a[NA];
#pragma unroll
    for (int k = 0; k < NA; ++k) a[k] = 0.0f;
    const bool rec = ep.active && t < E.t_max;
    if (ep.active) {
      float x[NO], raw[NA];
      es_normalise<NO>(nrm, mean, mdiff, o, x);
      es_net_step<KIND>(W, x, ring, t, raw);
#pragma unroll
      for (int k = 0; k < NA; ++k) a[k] = clip_action(raw[k]);
      if (rec) {
        const size_t row = (size_t)t * A.n + i;
#pragma unroll
        for (int k = 0; k < NO; ++k) { E.t_net_in[row * NO + k] = x[k]; E.t_obs[row * NO + k] = o[k]; }
#pragma unroll
        for (int k = 0; k < NA; ++k) { E.t_act[row * NA + k] = a[k]; E.t_raw[row * NA + k] = raw[k]; }
      }
    }
    int ns = 1;
    bool d = false, parked = false;
    float rew = env_wave_step<KIND, FORM>(Pl, s_hull, e, M, a, o, ns, d, parked, cnt TB_STAMP_PASS);
    if (ep.active) {
      end_agent_step<KIND, RG, false>(A, i, e, M, parked, ns, (size_t)i, o, d, cnt);  // (tb_es_evaluate claims a slot for every env)
      rew = tally_step(ep, t, rew, parked, d, e, M, cnt);
      if (rec) {
        E.t_rew[(size_t)t * A.n + i] = rew;
        E.t_done[(size_t)t * A.n + i] = d ? 1 : 0;
      }
    }
  }
  if (live) { E.ret[i] = ep.ret; E.len[i] = ep.len; }
  flush_counters(A.counters, cnt);
  TB_DIAG_STAMPS_END(st);
}

// SwingRacket: the 26th step's reward, written by the fast-forward into rew_last, completes the return (and the trace's row 25)
__global__ void __launch_bounds__(256) tb_es_fold_kernel(const float* rew_last, double* ret, int n, float* t_rew) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float r = rew_last[i];
  ret[i] += (double)r;
  if (t_rew) t_rew[(size_t)25 * n + i] = r;
}

}  // namespace

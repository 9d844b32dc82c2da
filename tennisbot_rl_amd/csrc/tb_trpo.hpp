// The TRPO learner's two kernels (tb_trpo_fvp, tb_trpo_search), built from the pieces of tb_learner.hpp (PpoLayout, PpoLayer,
// ppo_transpose, ppo_tanh / ppo_dtanh, tb_ppo_adv_stats_kernel, and its shared pieces ppo_tile, ppo_adv_norm, ppo_backward,
// ppo_partial_run / ppo_partial_total and PpoForward), and tb_trpo_returns' four at the end of the file, which need none of them. Device code only; included by tb_stepper.hip after tb_learner.hpp.
// The rule is the reference's agent.py (TRPOAgent; cited by line in tennisbot_rl_amd/trpo.py). Policy tower only: the LOG_STD,
// PI and PI_HEAD slots of the flat parameter vector. Every vector (v, F v, the search direction) is a full flat vector of
// PpoLayout::P floats; the value slots are ignored on input and written as 0. Instantiated per (kind, net) like the learner's kernels:
// both kinds' default nets and SwingRacket's [64, 64] (TB_NET_MLP64), which takes the NH == 2 paths of Tennisbot's default net.
//
// tb_trpo_fvp_kernel: F v = (1/m) sum_rows J^T diag(sigma^-2) J v over m rows of an index vector, J = d mean / d theta -- the
// Hessian of KL(old || new) at theta, which agent.py:144-167 obtains by double backprop (second-order and cross terms vanish at
// the expansion point). A workgroup of two waves takes TB_PPO_SHARE = 256 consecutive entries of the index vector, a wave one
// half, 16 rows per tile (ppo_tile), the shares of ppo_tower; waves never talk to each other. Per tile:
//   forward          h_l = tanh(W_l h_(l-1) + b_l)
//   tangent forward  zdot_l = V_l h_(l-1) + vb_l + W_l hdot_(l-1),  hdot_l = (1 - h_l^2) zdot_l;  mudot = V_H h + vb_H + W_H hdot
//                    (V, vb: v's slots of the layer, as weight fragments of their own beside W's. W's forward and transposed
//                    fragments and the dW accumulators fill the 512 registers of a lone wave, so V's fragments live in LDS:
//                    fragment f of lane l at [f][l], written and read by that lane alone -- no bank conflict, no barrier)
//   head             dout = sigma^-2 mudot
//   backward         ppo_backward: head, hidden layers, first layer (the operations of ppo_tower's own chain)
// Each wave writes its dW / db sums (an fp32 chain of 128 rows at the most) as one partial vector; tb_trpo_fvp_reduce_kernel
// adds the partials per parameter in float64 in a fixed order, divides by m and adds the damping. No float atomics.
//
// tb_trpo_search_kernel: forward only. Workgroup (share, k) takes candidate k and TB_TRPO_SEARCH_SHARE rows of the index
// vector; theta_k = theta + steps[k] * direction is formed while the fragments are loaded. The mean is computed with theta and
// with theta_k by the same code on the same inputs, so a zero step gives mu' == mu and KL == 0.0 exactly. Per workgroup one
// float64 pair (sum of ratio * A_hat, sum of KL); tb_trpo_search_reduce_kernel adds them in a fixed order: out[k] = the means.
#pragma once

namespace {

constexpr int TB_TRPO_SEARCH_SHARE = 1024;  // rows of the index vector per workgroup of the search: 4 waves of 16 tiles
constexpr int TB_TRPO_MAX_CANDIDATES = 64;

// PpoLayer plus the fragments of v's slots of the same layer (forward layout only: the backward pass is W's), kept in LDS
template <int IN, int OUT, bool FIRST>
struct TrpoLayer : PpoLayer<IN, OUT, FIRST> {
  using Base = PpoLayer<IN, OUT, FIRST>;
  static constexpr int NT = Base::NT, NTI = Base::NTI, NC = Base::NC;
  static constexpr int VF = NT * NC;  // fragments per lane
  const float* vf;                     // (t, c) at vf[(t NC + c) 64]: V[16 t + j][k(c, g)] of this lane
  f32x4 vbias[NT];

  // lds: VF * 64 floats of this wave's own
  TB_DEV void load_v(const float* V, const float* vb, int lane, float* lds) {
    const int g = lane >> 4, j = lane & 15;
    vf = lds + lane;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int o = 16 * t + j, k = FIRST ? 4 * c + g : 16 * (c >> 2) + 4 * g + (c & 3);
        lds[(t * NC + c) * 64 + lane] = (o < OUT && k < IN) ? V[o * IN + k] : 0.0f;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o = 16 * t + 4 * g + r;
        vbias[t][r] = o < OUT ? vb[o] : 0.0f;
      }
    }
  }
  // zdot = vb + V x (the observation has no tangent)
  TB_DEV void tangent_first(const float (&x)[NC], f32x4 (&zd)[NT]) const {
#pragma unroll
    for (int t = 0; t < NT; ++t) zd[t] = vbias[t];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
#pragma unroll
      for (int t = 0; t < NT; ++t) zd[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[(t * NC + c) * 64], x[c], zd[t], 0, 0, 0);
    }
  }
  // zdot = vb + V h + W hdot
  TB_DEV void tangent(const f32x4 (&h)[NTI], const f32x4 (&hd)[NTI], f32x4 (&zd)[NT]) const {
#pragma unroll
    for (int t = 0; t < NT; ++t) zd[t] = vbias[t];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
#pragma unroll
      for (int t = 0; t < NT; ++t) zd[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[(t * NC + c) * 64], h[c >> 2][c & 3], zd[t], 0, 0, 0);
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
#pragma unroll
      for (int t = 0; t < NT; ++t) zd[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(this->wf[t * NC + c], hd[c >> 2][c & 3], zd[t], 0, 0, 0);
    }
  }
};

struct TrpoFvpArgs {
  const float* obs;      // [N][O]
  const long long* idx;  // [m] rows (clamped)
  const float* params;   // [P]
  const float* vec;      // [P]
  float* partials;       // [2 * workgroups][P]
  long long n_rows;
  int m;
};

template <int KIND, int NET = TB_NET_DEFAULT>
__global__ __launch_bounds__(128) void tb_trpo_fvp_kernel(const TrpoFvpArgs a) {
  using L = PpoLayout<KIND, NET>;
  using N = PolicyNet<KIND, NET>;
  constexpr int O = L::O, NA = L::A, NH = L::NH;
  using L0 = TrpoLayer<O, N::H0, true>;
  using L1 = TrpoLayer<N::H0, N::H1, false>;
  using L2 = TrpoLayer<N::H1, N::H2, false>;  // (untouched when NH == 2)
  using LH = TrpoLayer<N::LAST, NA, false>;
  constexpr int VF = L0::VF + L1::VF + (NH == 3 ? L2::VF : 0) + LH::VF;
  __shared__ __attribute__((aligned(16))) float s_buf[2 * 512];
  __shared__ float s_vf[2 * VF * 64];
  const int lane = threadIdx.x & 63, half = threadIdx.x >> 6;
  const int first = blockIdx.x * TB_PPO_SHARE + half * TB_PPO_HALF;
  float* part = a.partials + (size_t)(2 * blockIdx.x + half) * L::P;
  float* buf = s_buf + half * 512;
  const int g = lane >> 4, B = a.m;
  const float* body = a.params + L::PI;
  const float* head = a.params + L::PI_HEAD;
  const float* vbody = a.vec + L::PI;
  const float* vhead = a.vec + L::PI_HEAD;
  L0 l0;
  L1 l1;
  L2 l2;
  LH lh;
  float* vl = s_vf + half * (VF * 64);
  l0.load(body + L::W0, body + L::B0, lane); l0.load_v(vbody + L::W0, vbody + L::B0, lane, vl);
  l1.load(body + L::W1, body + L::B1, lane); l1.load_v(vbody + L::W1, vbody + L::B1, lane, vl + 64 * L0::VF);
  if (NH == 3) { l2.load(body + L::W2, body + L::B2, lane); l2.load_v(vbody + L::W2, vbody + L::B2, lane, vl + 64 * (L0::VF + L1::VF)); }
  lh.load(head, head + NA * N::LAST, lane); lh.load_v(vhead, vhead + NA * N::LAST, lane, vl + 64 * (VF - LH::VF));
  float inv_var[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) inv_var[r] = 4 * g + r < NA ? expf(-2.0f * a.params[L::LOG_STD + 4 * g + r]) : 0.0f;

  for (int i0 = first; i0 < first + TB_PPO_HALF && i0 < B; i0 += 16) {
    bool valid;
    float x0[L0::NC];
    f32x4 obsT[1];
    ppo_tile<O>(a.obs, a.idx, i0, B, a.n_rows, lane, valid, x0, obsT);
    // forward and tangent forward, layer by layer
    f32x4 z0[L0::NT], h0[L0::NT], hd0[L0::NT], z1[L1::NT], h1[L1::NT], hd1[L1::NT], z2[L2::NT], h2[L2::NT], hd2[L2::NT], mud[1];
    l0.forward_first(x0, z0); ppo_tanh(z0, h0);
    l0.tangent_first(x0, z0); ppo_dtanh(z0, h0, hd0);
    l1.forward(h0, z1); ppo_tanh(z1, h1);
    l1.tangent(h0, hd0, z1); ppo_dtanh(z1, h1, hd1);
    if constexpr (NH == 3) {
      l2.forward(h1, z2); ppo_tanh(z2, h2);
      l2.tangent(h1, hd1, z2); ppo_dtanh(z2, h2, hd2);
      lh.tangent(h2, hd2, mud);
    } else {
      lh.tangent(h1, hd1, mud);
    }
    f32x4 dout[1];
#pragma unroll
    for (int r = 0; r < 4; ++r) dout[0][r] = (valid && 4 * g + r < NA) ? mud[0][r] * inv_var[r] : 0.0f;
    ppo_backward<NH>(l0, l1, l2, lh, dout, obsT, h0, h1, h2, buf, lane);
  }
  float* gbody = part + L::PI;
  float* ghead = part + L::PI_HEAD;
  l0.store(gbody + L::W0, gbody + L::B0, lane);
  l1.store(gbody + L::W1, gbody + L::B1, lane);
  if (NH == 3) l2.store(gbody + L::W2, gbody + L::B2, lane);
  lh.store(ghead, ghead + NA * N::LAST, lane);
}

// out[p] = (float)(sum of the partials / m) + damping v[p] on the network's policy slots (ppo_partial_run / ppo_partial_total's float64 sum;
// the two float32 roundings of the damping term are separate: fvp(d) == fvp(0) + fl(d v) bit for bit),
// 2 v[p] + damping v[p] on log_std (the Gaussian's own Fisher block: exact), 0 on the value slots. 64 parameters per block.
template <int KIND, int NET = TB_NET_DEFAULT>
__global__ __launch_bounds__(256) void tb_trpo_fvp_reduce_kernel(const float* partials, int n_part, int m, const float* vec, float damping, float* out) {
  using L = PpoLayout<KIND, NET>;
  __shared__ double s_sum[4][64];
  const int j = threadIdx.x & 63, q = threadIdx.x >> 6, p = blockIdx.x * 64 + j;
  const bool net = (p >= L::PI && p < L::VF) || (p >= L::PI_HEAD && p < L::VF_HEAD);
  s_sum[q][j] = net ? ppo_partial_run(partials, L::P, p, n_part, q) : 0.0;
  __syncthreads();
  if (q == 0 && p < L::P) {
    const double total = ppo_partial_total(s_sum, j);
    const float v = vec[p];
    out[p] = net ? (float)(total / (double)m) + damping * v : p < L::A ? 2.0f * v + damping * v : 0.0f;
  }
}

// --------------------------------------------------------------------------------------------------------------- line search
// forward fragments of theta + step * direction for one nn.Linear
template <int IN, int OUT, bool FIRST>
struct TrpoFwd : PpoForward<IN, OUT, FIRST> {
  using Fwd = PpoForward<IN, OUT, FIRST>;
  using Fwd::wf;
  using Fwd::bias;
  static constexpr int NT = Fwd::NT, NC = Fwd::NC;
  static_assert(FIRST || IN % 16 == 0, "the search is built for hidden widths that are whole tiles: NC = IN / 4");
  TB_DEV void load(const float* W, const float* b, const float* DW, const float* Db, float step, int lane) {
    const int g = lane >> 4, j = lane & 15;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int o = 16 * t + j, k = FIRST ? 4 * c + g : 16 * (c >> 2) + 4 * g + (c & 3);
        wf[t * NC + c] = (o < OUT && k < IN) ? W[o * IN + k] + step * DW[o * IN + k] : 0.0f;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o = 16 * t + 4 * g + r;
        bias[t][r] = o < OUT ? b[o] + step * Db[o] : 0.0f;
      }
    }
  }
};

// the policy tower's forward pass at theta + step * direction
template <int KIND, int NET = TB_NET_DEFAULT>
struct TrpoMean {
  using L = PpoLayout<KIND, NET>;
  using N = PolicyNet<KIND, NET>;
  using L0 = TrpoFwd<L::O, N::H0, true>;
  using L1 = TrpoFwd<N::H0, N::H1, false>;
  using L2 = TrpoFwd<N::H1, N::H2, false>;
  using LH = TrpoFwd<N::LAST, L::A, false>;
  L0 l0;
  L1 l1;
  L2 l2;
  LH lh;
  TB_DEV void load(const float* params, const float* dir, float step, int lane) {
    const float *body = params + L::PI, *head = params + L::PI_HEAD, *dbody = dir + L::PI, *dhead = dir + L::PI_HEAD;
    l0.load(body + L::W0, body + L::B0, dbody + L::W0, dbody + L::B0, step, lane);
    l1.load(body + L::W1, body + L::B1, dbody + L::W1, dbody + L::B1, step, lane);
    if (L::NH == 3) l2.load(body + L::W2, body + L::B2, dbody + L::W2, dbody + L::B2, step, lane);
    lh.load(head, head + L::A * N::LAST, dhead, dhead + L::A * N::LAST, step, lane);
  }
  TB_DEV f32x4 mean(const float (&x0)[L0::NC]) const {
    f32x4 z0[L0::NT], h0[L0::NT], z1[L1::NT], h1[L1::NT], zh[1];
    l0.forward_first(x0, z0); ppo_tanh(z0, h0);
    l1.forward(h0, z1); ppo_tanh(z1, h1);
    if constexpr (L::NH == 3) {
      f32x4 z2[L2::NT], h2[L2::NT];
      l2.forward(h1, z2); ppo_tanh(z2, h2);
      lh.forward(h2, zh);
    } else {
      lh.forward(h1, zh);
    }
    return zh[0];
  }
};

struct TrpoSearchArgs {
  const float* obs;        // [N][O]
  const float* act;        // [N][A] the unclipped samples
  const float* old_logp;   // [N]
  const float* adv;        // [N]
  const long long* idx;    // [B]
  const float* params;     // [P]
  const float* dir;        // [P]
  const float* steps;      // [K]
  const double* adv_sums;  // [TB_PPO_STAT_BLOCKS][2]
  double* partials;        // [K][shares][2]
  long long n_rows;
  int batch;
};

template <int KIND, int NET = TB_NET_DEFAULT>
__global__ __launch_bounds__(256) void tb_trpo_search_kernel(const TrpoSearchArgs a) {
  using L = PpoLayout<KIND, NET>;
  constexpr int O = L::O, NA = L::A;
  __shared__ double s_part[4][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, B = a.batch;
  const int first = blockIdx.x * TB_TRPO_SEARCH_SHARE + wave * (TB_TRPO_SEARCH_SHARE / 4);
  const float step = a.steps[blockIdx.y];
  TrpoMean<KIND, NET> cur, cand;
  cur.load(a.params, a.dir, 0.0f, lane);
  cand.load(a.params, a.dir, step, lane);
  const PpoAdvNorm norm = ppo_adv_norm(a.adv_sums, B);
  float dls[4], ls2[4], inv_std2[4], e2[4], inv_var2[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const bool on = 4 * g + r < NA;
    const float ls = on ? a.params[L::LOG_STD + 4 * g + r] : 0.0f;
    ls2[r] = on ? ls + step * a.dir[L::LOG_STD + 4 * g + r] : 0.0f;
    dls[r] = ls2[r] - ls;
    inv_std2[r] = expf(-ls2[r]);
    e2[r] = expf(-2.0f * dls[r]);       // sigma^2 / sigma'^2
    inv_var2[r] = expf(-2.0f * ls2[r]);
  }
  double sum_l = 0.0, sum_kl = 0.0;  // this lane's rows (lanes of group 0 only)
  for (int i0 = first; i0 < first + TB_TRPO_SEARCH_SHARE / 4 && i0 < B; i0 += 16) {
    bool valid;
    float x0[TrpoMean<KIND, NET>::L0::NC];
    const long long row = ppo_tile<O>(a.obs, a.idx, i0, B, a.n_rows, lane, valid, x0);
    const f32x4 mu = cur.mean(x0), mu2 = cand.mean(x0);
    float lp = 0.0f, kl = 0.0f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (4 * g + r < NA) {
        const float zeta = (a.act[(size_t)row * NA + 4 * g + r] - mu2[r]) * inv_std2[r];
        lp += (-0.5f * zeta * zeta - ls2[r]) - TB_LN_SQRT_2PI;
        const float d = mu[r] - mu2[r];
        kl += (dls[r] + 0.5f * (e2[r] + (d * d) * inv_var2[r])) - 0.5f;
      }
    }
    lp += __shfl_xor(lp, 16); lp += __shfl_xor(lp, 32);
    kl += __shfl_xor(kl, 16); kl += __shfl_xor(kl, 32);
    const float ratio = expf(lp - a.old_logp[row]);
    const float an = (a.adv[row] - norm.mean) / norm.den;
    if (valid && g == 0) { sum_l += (double)(ratio * an); sum_kl += (double)kl; }
  }
#pragma unroll
  for (int w = 1; w < 16; w <<= 1) { sum_l += __shfl_xor(sum_l, w); sum_kl += __shfl_xor(sum_kl, w); }
  if (lane == 0) { s_part[wave][0] = sum_l; s_part[wave][1] = sum_kl; }
  __syncthreads();
  if (threadIdx.x < 2) {
    const int c = threadIdx.x;
    a.partials[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2 + c] = (s_part[0][c] + s_part[1][c]) + (s_part[2][c] + s_part[3][c]);
  }
}

// out[k] = (mean of ratio A_hat, mean KL) of candidate k = blockIdx.x: the workgroups' pairs in a fixed order
__global__ __launch_bounds__(256) void tb_trpo_search_reduce_kernel(const double* partials, int shares, int batch, double* out) {
  __shared__ double s_l[256], s_k[256];
  const double* p = partials + (size_t)blockIdx.x * shares * 2;
  double l = 0.0, k = 0.0;
  for (int s = threadIdx.x; s < shares; s += 256) { l += p[2 * s]; k += p[2 * s + 1]; }
  s_l[threadIdx.x] = l; s_k[threadIdx.x] = k;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) { s_l[threadIdx.x] += s_l[threadIdx.x + w]; s_k[threadIdx.x] += s_k[threadIdx.x + w]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { out[2 * blockIdx.x] = s_l[0] / (double)batch; out[2 * blockIdx.x + 1] = s_k[0] / (double)batch; }
}

// ------------------------------------------------------------------------------------- discounted returns of finished episodes
// agent.py's estimator (agent.py:193-230, 264-268): no critic, the surrogate is weighted by the discounted return-to-go of the
// episodes that ENDED inside the rollout. Row (t, e) is finished iff t <= L_e, L_e the last step of env e with done != 0 (-1: none).
// Four launches, integers and exactly rounded float64 only, no atomics: the same inputs give the same bits.
//
// tb_trpo_returns_kernel: one lane per env, backwards over the steps as tb_ppo_gae_kernel (a step's loads and stores coalesce
// across envs and do not depend on the chain). R = r where done, else r + discount R', carried in float64 -- the product and the
// sum rounded separately (__dmul_rn / __dadd_rn are never contracted) -- and rounded to float32 once, at the store; 0.0f on
// unfinished rows. Writes L_e.
// tb_trpo_finished_count_kernel: one wave per (step, 64-env chunk) ballots t <= L_e; its population count goes to table[t][chunk].
// tb_trpo_finished_scan_kernel: ONE workgroup turns the table into exclusive offsets in row-major order, 1024 entries per pass
// (wave scan by shuffles, the 16 wave totals through LDS, a running carry); the total is *count.
// tb_trpo_finished_scatter_kernel: the count kernel's wave shape again; a set lane writes t n + e to idx[offset + set lanes below it].
__global__ __launch_bounds__(64) void tb_trpo_returns_kernel(int T, int n, const float* rew, size_t rew_stride, const unsigned char* done, size_t done_stride,
                                                             double discount, float* ret, int* last) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  double R = 0.0;
  int L = -1;
#pragma unroll 8
  for (int k = T - 1; k >= 0; --k) {
    const bool d = done[(size_t)k * done_stride + i] != 0;
    const double r = (double)rew[(size_t)k * rew_stride + i];
    R = d ? r : __dadd_rn(r, __dmul_rn(discount, R));
    L = (d && L < 0) ? k : L;
    ret[(size_t)k * n + i] = L >= 0 ? (float)R : 0.0f;
  }
  last[i] = L;
}

// wave w of the grid takes table entry w = t * chunks + chunk; 4 waves per workgroup
TB_DEV bool trpo_finished_lane(int T, int chunks, long long& w, int& t, int& e) {
  w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= (long long)T * chunks) return false;  // (the whole wave leaves: w is wave-uniform)
  t = (int)(w / chunks);
  e = (int)(w % chunks) * 64 + (int)(threadIdx.x & 63);
  return true;
}

__global__ __launch_bounds__(256) void tb_trpo_finished_count_kernel(int T, int n, int chunks, const int* last, long long* table) {
  long long w;
  int t, e;
  if (!trpo_finished_lane(T, chunks, w, t, e)) return;
  const unsigned long long set = __ballot(e < n && t <= last[e < n ? e : n - 1]);
  if ((threadIdx.x & 63) == 0) table[w] = (long long)__popcll(set);
}

__global__ __launch_bounds__(1024) void tb_trpo_finished_scan_kernel(long long entries, long long* table, long long* count) {
  __shared__ long long s_wave[16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long long carry = 0;
  for (long long base = 0; base < entries; base += 1024) {
    const long long i = base + threadIdx.x;
    const long long own = i < entries ? table[i] : 0;
    long long incl = own;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const long long up = __shfl_up(incl, d);
      if (lane >= d) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    long long before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const long long s = s_wave[k];
      before += k < wave ? s : 0;
      total += s;
    }
    if (i < entries) table[i] = carry + before + (incl - own);
    carry += total;
    __syncthreads();  // s_wave is written again in the next pass
  }
  if (threadIdx.x == 0) *count = carry;
}

__global__ __launch_bounds__(256) void tb_trpo_finished_scatter_kernel(int T, int n, int chunks, const int* last, const long long* table, long long* idx) {
  long long w;
  int t, e;
  if (!trpo_finished_lane(T, chunks, w, t, e)) return;
  const bool on = e < n && t <= last[e < n ? e : n - 1];
  const unsigned long long set = __ballot(on);
  const unsigned below = __builtin_amdgcn_mbcnt_hi((unsigned)(set >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)set, 0u));
  if (on) idx[table[w] + (long long)below] = (long long)t * n + e;
}

}  // namespace

// The SAC learner's kernels (C ABI tb_sac_* in include/tb_stepper.h; tennisbot_rl_amd/sac.py is the caller). Device code only;
// included by tb_stepper.hip after tb_learner.hpp (f32x4, TB_DEV, TB_LN_SQRT_2PI).
//
// SB3's SAC nets are [256, 256] ReLU towers: one 256 x 256 fp32 layer is 256 KiB, twice a wave's register file, so the
// register-resident towers of PpoLayer do not apply. The form here is output-stationary instead: every matrix product of the
// step is one launch in which a wave owns ONE 16 x 16 tile of the result and runs the reduction index in steps of four on the
// f32-input MFMA (v_mfma_f32_16x16x4_f32: exact fp32 products, fp32 accumulation), operands read straight from global memory
// (weights and activations of a step are L2-resident). Three tile kernels cover actor, critic and target, forward and backward:
//   sac_forward_kernel   Y[b][o] = act(b[o] + sum_k X[b][k] W[o][k])               reduction over the layer's inputs
//   sac_backward_kernel  dX[b][k] = [H[b][k] > 0] sum_o dZ[b][o] W[o][k]           reduction over the layer's outputs
//   sac_wgrad_kernel     dW[o][k] = sum_b dZ[b][o] H[b][k], db[o] = sum_b dZ[b][o] reduction over the batch rows IN INDEX ORDER
// blockIdx.z selects one of two nets of equal shape (qf0 / qf1, the two targets, or the actor's mu / log_std heads, which are
// two [A][256] + [A] blocks one after the other in the flat vector). The weight gradient needs no partial vectors and no
// reduction kernel: a tile's sum over the rows is one fp32 MFMA chain in one fixed order. Activations H (post-ReLU; H > 0 is
// the ReLU mask) and dZ are [B][256] in the workspace. Row-wise work (gather through the index vector, sample and logp,
// targets, losses, the tanh / logp backward) is in small kernels of one thread per row; the two losses and the entropy
// coefficient's gradient are float64 sums in a fixed tree order. No float atomics; every loop is bounded by its arguments;
// a stage that needs another's complete output is a later launch on the same stream.
//
// Episode ends: the envs carry no time limit, so done == 1 is a true terminal and removes the bootstrap; the stored next_obs of
// such a row is the next episode's first observation (auto-reset), finite, and selected away: y = r bit for bit.
#pragma once

namespace {

constexpr int SAC_H = 256;           // hidden width
constexpr int SAC_XW = 16;           // padded width of a net's input rows and of the head rows in the workspace
constexpr int SAC_ROWS_PER_WG = 64;  // four waves of one 16-row tile each
constexpr int SAC_UNROLL = 8;        // MFMA steps of a tile kernel whose loads are issued together
constexpr float SAC_LOG_STD_MIN = -20.0f, SAC_LOG_STD_MAX = 2.0f, SAC_SQUASH_EPS = 1e-6f;

template <int KIND> struct SacLayout {
  static constexpr int O = KIND == TB_ENV_SWING ? 6 : 12, A = KIND == TB_ENV_SWING ? 6 : 2, C = O + A;
  // actor: latent_pi.0 W b | latent_pi.2 W b | mu W b | log_std W b
  static constexpr int PI_W0 = 0, PI_B0 = PI_W0 + SAC_H * O, PI_W1 = PI_B0 + SAC_H, PI_B1 = PI_W1 + SAC_H * SAC_H, PI_HEAD = PI_B1 + SAC_H;
  static constexpr int PI_HEAD_BLOCK = A * SAC_H + A, PI_P = PI_HEAD + 2 * PI_HEAD_BLOCK;
  // one critic: W0 [256][O + A] b0 | W1 b1 | W2 [1][256] b2; the flat vector holds qf0 then qf1
  static constexpr int Q_W0 = 0, Q_B0 = Q_W0 + SAC_H * C, Q_W1 = Q_B0 + SAC_H, Q_B1 = Q_W1 + SAC_H * SAC_H, Q_W2 = Q_B1 + SAC_H, Q_B2 = Q_W2 + SAC_H;
  static constexpr int Q_ONE = Q_B2 + 1, Q_P = 2 * Q_ONE;
};
static_assert(SacLayout<TB_ENV_SWING>::PI_P == 70668 && SacLayout<TB_ENV_TENNIS>::PI_P == 70148, "actor parameter count");
static_assert(SacLayout<TB_ENV_SWING>::Q_P == 138754 && SacLayout<TB_ENV_TENNIS>::Q_P == 139778, "critic parameter count");

// The workspace: per batch row these many floats, region by region (each region is [B][width], or [2][B][width] for two nets).
// HW is the padded width of a critic's head rows (QT, Q, DQ); ROW_SUM the floats per row of the critic loss's row sums (RL).
template <int HW, int ROW_SUM> struct SacWsT {
  // stage (a), kept until stage (d): actor on s
  static constexpr int X0 = 0, H1 = X0 + 16, H2 = H1 + 256, ZH = H2 + 256, XC = ZH + 16, LP = XC + 16;
  // stage (b): actor on s', targets on (s', a')
  static constexpr int NX0 = LP + 16, NH1 = NX0 + 16, NH2 = NH1 + 256, NZH = NH2 + 256, NXC = NZH + 16, NAL = NXC + 16, T1 = NAL + 16, T2 = T1 + 512, QT = T2 + 512;
  // stages (c) and (d): the critics on (s, a), then on (s, a~)
  static constexpr int XSA = QT + 2 * HW, C1 = XSA + 16, C2 = C1 + 512, Q = C2 + 512, DQ = Q + 2 * HW, DZ2 = DQ + 2 * HW, DZ1 = DZ2 + 512;
  // stage (d): the critics' input gradient, the actor's backward pass
  static constexpr int DX = DZ1 + 512, DHD = DX + 32, DA2 = DHD + 16, DA1 = DA2 + 256, RL = DA1 + 256, PER_ROW = RL + ROW_SUM;
};
using SacWs = SacWsT<SAC_XW, 0>;
static_assert(SacWs::QT == 2176 && SacWs::Q == 3248 && SacWs::DQ == 3280 && SacWs::DX == 4336 && SacWs::PER_ROW == 4896, "SAC's workspace layout");

TB_DEV long long sac_row(const long long* idx, int b, long long n_rows) {
  long long r = idx[b];
  return r < 0 ? 0 : r >= n_rows ? n_rows - 1 : r;
}

// ---------------------------------------------------------------------------------------------------------------- tile kernels
struct SacFwdArgs {
  const float* x; int xs; long long xz;  // X[b][k] at x[z xz + b xs + k]
  const float* w; int wrs; long long wz; // W[o][k] at w[z wz + o wrs + k]
  const float* bias;                     // b[o] at bias[z wz + o]
  float* y; int ys; long long yz;        // Y[b][o] at y[z yz + b ys + o]
  int B, K, M;                           // rows, inputs, outputs
};

// grid (ceil(B / 64), ceil(M / 16), nets), 256 threads: wave w of block x takes rows 64 x + 16 w ..
template <bool RELU>
__global__ __launch_bounds__(256) void sac_forward_kernel(const SacFwdArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, e = lane & 15, z = blockIdx.z;
  const int b0 = blockIdx.x * SAC_ROWS_PER_WG + 16 * wave, o0 = blockIdx.y * 16;
  if (b0 >= a.B) return;
  const float* x = a.x + z * a.xz;
  const float* w = a.w + z * a.wz;
  const int o = o0 + e, b = b0 + e;
  const bool o_in = o < a.M, b_in = b < a.B;
  const float* wrow = w + (size_t)(o_in ? o : 0) * a.wrs;
  const float* xrow = x + (size_t)(b_in ? b : 0) * a.xs;
  f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
  int k0 = 0;
  for (; k0 + 4 * SAC_UNROLL <= a.K; k0 += 4 * SAC_UNROLL) {  // whole chunks: SAC_UNROLL independent loads in flight, no bound on k
    float wl[SAC_UNROLL], xl[SAC_UNROLL];
#pragma unroll
    for (int u = 0; u < SAC_UNROLL; ++u) { wl[u] = wrow[k0 + 4 * u + g]; xl[u] = xrow[k0 + 4 * u + g]; }
#pragma unroll
    for (int u = 0; u < SAC_UNROLL; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(o_in ? wl[u] : 0.0f, b_in ? xl[u] : 0.0f, acc, 0, 0, 0);
  }
  for (; k0 < a.K; k0 += 4) {
    const int k = k0 + g, kc = k < a.K ? k : a.K - 1;  // (every address is a valid one; what lies outside is selected away)
    const bool k_in = k < a.K;
    const float wl = wrow[kc], xl = xrow[kc];
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32((o_in && k_in) ? wl : 0.0f, (b_in && k_in) ? xl : 0.0f, acc, 0, 0, 0);  // acc[r]: output o0 + 4 g + r of row b0 + e
  }
  if (!b_in) return;
  float* yrow = a.y + z * a.yz + (size_t)b * a.ys;
  const float* bias = a.bias + z * a.wz;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int oo = o0 + 4 * g + r;
    if (oo < a.M) {
      const float v = acc[r] + bias[oo];
      yrow[oo] = RELU ? fmaxf(v, 0.0f) : v;
    }
  }
}

struct SacBwdArgs {
  const float* dz; int dzs; long long dzz;  // dZ[b][o] at dz[z dzz + b dzs + o]
  const float* w; int wrs; long long wz;    // W[o][k] at w[z wz + o wrs + k]
  int split, split_extra;                   // rows o >= split lie split_extra floats further on (the actor's two head blocks)
  const float* h; int hs; long long hz;     // the ReLU mask: H[b][k] > 0 (MASK only)
  float* dx; int dxs; long long dxz;        // dX[b][k] at dx[z dxz + b dxs + k]
  int B, K, M;                              // rows, the layer's inputs (result columns), the layer's outputs (reduction)
};

// grid (ceil(B / 64), ceil(K / 16), nets), 256 threads
template <bool MASK>
__global__ __launch_bounds__(256) void sac_backward_kernel(const SacBwdArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, e = lane & 15, z = blockIdx.z;
  const int b0 = blockIdx.x * SAC_ROWS_PER_WG + 16 * wave, k0 = blockIdx.y * 16;
  if (b0 >= a.B) return;
  const float* w = a.w + z * a.wz;
  const int k = k0 + e, b = b0 + e;
  const bool k_in = k < a.K, b_in = b < a.B;
  const int kc = k_in ? k : 0;
  const float* dzrow = a.dz + z * a.dzz + (size_t)(b_in ? b : 0) * a.dzs;
  f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
  int o0 = 0;
  for (; o0 + 4 * SAC_UNROLL <= a.M; o0 += 4 * SAC_UNROLL) {
    float wl[SAC_UNROLL], dl[SAC_UNROLL];
#pragma unroll
    for (int u = 0; u < SAC_UNROLL; ++u) {
      const int o = o0 + 4 * u + g;
      wl[u] = w[(size_t)o * a.wrs + (o >= a.split ? a.split_extra : 0) + kc];
      dl[u] = dzrow[o];
    }
#pragma unroll
    for (int u = 0; u < SAC_UNROLL; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(k_in ? wl[u] : 0.0f, b_in ? dl[u] : 0.0f, acc, 0, 0, 0);
  }
  for (; o0 < a.M; o0 += 4) {
    const int o = o0 + g, oc = o < a.M ? o : a.M - 1;
    const bool o_in = o < a.M;
    const float wl = w[(size_t)oc * a.wrs + (oc >= a.split ? a.split_extra : 0) + kc], dl = dzrow[oc];
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32((o_in && k_in) ? wl : 0.0f, (o_in && b_in) ? dl : 0.0f, acc, 0, 0, 0);  // acc[r]: input k0 + 4 g + r of row b0 + e
  }
  if (!b_in) return;
  float* dxrow = a.dx + z * a.dxz + (size_t)b * a.dxs;
  const float* hrow = MASK ? a.h + z * a.hz + (size_t)b * a.hs : nullptr;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int kk = k0 + 4 * g + r;
    if (kk < a.K) dxrow[kk] = MASK ? (hrow[kk] > 0.0f ? acc[r] : 0.0f) : acc[r];
  }
}

struct SacWgradArgs {
  const float* dz; int dzs; long long dzz;  // dZ[b][o]
  const float* h; int hs; long long hz;     // H[b][k]: the layer's input
  float* gw; int wrs; long long wz;         // dW[o][k] at gw[z wz + o wrs + k]
  float* gb;                                // db[o] at gb[z wz + o]
  int B, K, M;
};

// grid (ceil(K / 64), ceil(M / 16), nets), 256 threads: wave w takes input columns 64 x + 16 w ..; the tile of column 0 also sums db
__global__ __launch_bounds__(256) void sac_wgrad_kernel(const SacWgradArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, e = lane & 15, z = blockIdx.z;
  const int k0 = blockIdx.x * 64 + 16 * wave, o0 = blockIdx.y * 16;
  if (k0 >= a.K) return;
  const float* dz = a.dz + z * a.dzz;
  const float* h = a.h + z * a.hz;
  const int o = o0 + e, k = k0 + e;
  const bool o_in = o < a.M, k_in = k < a.K, with_bias = k0 == 0;
  const int oc = o_in ? o : 0, kc = k_in ? k : 0;
  f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f}, accb = {0.0f, 0.0f, 0.0f, 0.0f};
  int r0 = 0;
  for (; r0 + 4 * SAC_UNROLL <= a.B; r0 += 4 * SAC_UNROLL) {
    float dl[SAC_UNROLL], hl[SAC_UNROLL];
#pragma unroll
    for (int u = 0; u < SAC_UNROLL; ++u) {
      const int b = r0 + 4 * u + g;
      dl[u] = dz[(size_t)b * a.dzs + oc];
      hl[u] = h[(size_t)b * a.hs + kc];
    }
#pragma unroll
    for (int u = 0; u < SAC_UNROLL; ++u) {
      const float dv = o_in ? dl[u] : 0.0f;
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(dv, k_in ? hl[u] : 0.0f, acc, 0, 0, 0);
      if (with_bias) accb = __builtin_amdgcn_mfma_f32_16x16x4f32(dv, 1.0f, accb, 0, 0, 0);
    }
  }
  for (; r0 < a.B; r0 += 4) {
    const int b = r0 + g, bc = b < a.B ? b : a.B - 1;
    const bool b_in = b < a.B;
    const float dl = dz[(size_t)bc * a.dzs + oc], hl = h[(size_t)bc * a.hs + kc];
    const float dv = (b_in && o_in) ? dl : 0.0f;
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(dv, (b_in && k_in) ? hl : 0.0f, acc, 0, 0, 0);  // acc[r]: dW[o0 + 4 g + r][k0 + e]
    if (with_bias) accb = __builtin_amdgcn_mfma_f32_16x16x4f32(dv, 1.0f, accb, 0, 0, 0);
  }
  float* gw = a.gw + z * a.wz;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int oo = o0 + 4 * g + r;
    if (oo < a.M) {
      if (k_in) gw[(size_t)oo * a.wrs + k] = acc[r];
      if (with_bias && e == 0) a.gb[z * a.wz + oo] = accb[r];
    }
  }
}

// ----------------------------------------------------------------------------------------------------------------- row kernels
// out[b][0 .. 16) = obs[row][0 .. O) | act[row][0 .. A) (or nothing) | 0, row = the clamped idx[b]
__global__ __launch_bounds__(256) void sac_gather_kernel(const float* obs, int O, const float* act, int A, const long long* idx, long long n_rows, int B, float* out) {
  const int i = blockIdx.x * 256 + threadIdx.x, b = i >> 4, c = i & 15;
  if (b >= B) return;
  const long long row = sac_row(idx, b, n_rows);
  float v = 0.0f;
  if (c < O) v = obs[(size_t)row * O + c];
  else if (act && c < O + A) v = act[(size_t)row * A + (c - O)];
  out[(size_t)b * SAC_XW + c] = v;
}

// one thread per row: the squashed sample and its log-probability from the head's outputs zh[b] = mu [A] | log_std [A];
// xc[b] = the row's observation | the sample | 0: the critics' input; lp[b][0] = logp. act_out / logp_out may be null
__global__ __launch_bounds__(256) void sac_sample_kernel(const float* x0, const float* zh, const float* eps, int O, int A, int B, float* act_out, float* logp_out, float* xc,
                                                         float* lp) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const float* z = zh + (size_t)b * SAC_XW;
  float* xr = xc + (size_t)b * SAC_XW;
  float s_gauss = 0.0f, s_squash = 0.0f;
  for (int c = 0; c < SAC_XW; ++c) xr[c] = c < O ? x0[(size_t)b * SAC_XW + c] : 0.0f;
  for (int j = 0; j < A; ++j) {
    const float ls = fminf(fmaxf(z[A + j], SAC_LOG_STD_MIN), SAC_LOG_STD_MAX), ep = eps[(size_t)b * A + j];
    const float gs = z[j] + expf(ls) * ep;
    const float t = tanhf(gs);
    s_gauss += (-0.5f * ep * ep - ls) - TB_LN_SQRT_2PI;
    s_squash += logf((1.0f - t * t) + SAC_SQUASH_EPS);
    xr[O + j] = t;
    if (act_out) act_out[(size_t)b * A + j] = t;
  }
  const float logp = s_gauss - s_squash;
  if (logp_out) logp_out[b] = logp;
  lp[(size_t)b * SAC_XW] = logp;
}

// y = r + (1 - d) gamma (min(Q1t, Q2t) - alpha logp'); a terminal row is selected, not multiplied: y = r bit for bit
__global__ __launch_bounds__(256) void sac_target_kernel(const float* reward, const float* done, const long long* idx, long long n_rows, int B, const float* qt,
                                                         const float* logp_next, const float* log_ent_coef, float gamma, float* y) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const long long row = sac_row(idx, b, n_rows);
  const float alpha = expf(log_ent_coef[0]);
  const float q = fminf(qt[(size_t)b * SAC_XW], qt[(size_t)(B + b) * SAC_XW]);
  const float r = reward[row];
  y[b] = done[row] != 0.0f ? r : r + gamma * (q - alpha * logp_next[(size_t)b * SAC_XW]);
}

// one workgroup: float64 sum of 256 strided per-thread sums, then a tree: one fixed order
TB_DEV double sac_block_sum(double v, double* s) {
  s[threadIdx.x] = v;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
    __syncthreads();
  }
  const double out = s[0];
  __syncthreads();
  return out;
}

// dq[n][b] = (Q_n(s, a)[b] - y[b]) / B; stats[0] = 0.5 (mean d1^2 + mean d2^2). One workgroup.
__global__ __launch_bounds__(256) void sac_critic_loss_kernel(const float* q, const float* y, int B, float* dq, double* stats) {
  __shared__ double s[256];
  double sq = 0.0;
  const float inv = 1.0f / (float)B;
  for (int b = threadIdx.x; b < B; b += 256) {
    for (int n = 0; n < 2; ++n) {
      const float d = q[(size_t)(n * B + b) * SAC_XW] - y[b];
      dq[(size_t)(n * B + b) * SAC_XW] = d * inv;
      sq += (double)d * (double)d;
    }
  }
  const double total = sac_block_sum(sq, s);
  if (threadIdx.x == 0) stats[0] = 0.5 * total / (double)B;
}

// the actor loss mean(alpha logp - min(Q1, Q2)(s, a~)): dq[n][b] = -1 / B on the smaller critic, 0 on the other (Q1 on a tie);
// stats[1] = the loss, stats[2] = mean logp, stats[3] = the gradient of log_ent_coef, -mean(logp + target_entropy), also
// written as float32 to ent_grad. One workgroup.
__global__ __launch_bounds__(256) void sac_actor_loss_kernel(const float* q, const float* lp, const float* log_ent_coef, float target_entropy, int B, float* dq,
                                                             float* ent_grad, double* stats) {
  __shared__ double s[256];
  const float alpha = expf(log_ent_coef[0]), inv = 1.0f / (float)B;
  double sl = 0.0, sp = 0.0, se = 0.0;
  for (int b = threadIdx.x; b < B; b += 256) {
    const float q0 = q[(size_t)b * SAC_XW], q1 = q[(size_t)(B + b) * SAC_XW], logp = lp[(size_t)b * SAC_XW];
    const bool first = q0 <= q1;
    dq[(size_t)b * SAC_XW] = first ? -inv : 0.0f;
    dq[(size_t)(B + b) * SAC_XW] = first ? 0.0f : -inv;
    sl += (double)(alpha * logp - (first ? q0 : q1));
    sp += (double)logp;
    se += (double)(logp + target_entropy);
  }
  const double tl = sac_block_sum(sl, s), tp = sac_block_sum(sp, s), te = sac_block_sum(se, s);
  if (threadIdx.x == 0) {
    stats[1] = tl / (double)B;
    stats[2] = tp / (double)B;
    stats[3] = -te / (double)B;
    ent_grad[0] = (float)(-te / (double)B);
  }
}

// one thread per (row, action): the loss's gradient with respect to the head's outputs, through a~ = tanh(g), g = mu + sigma eps:
//   dL/dg = da (1 - a~^2) + c 2 a~ (1 - a~^2) / (1 - a~^2 + 1e-6),  c = alpha / B,  da = both critics' input gradients summed
//   dL/dmu = dL/dg,  dL/dlog_std = dL/dg sigma eps - c, zero where the clamp binds (outside [-20, 2])
__global__ __launch_bounds__(256) void sac_head_backward_kernel(const float* zh, const float* xc, const float* dx, const float* eps, const float* log_ent_coef, int O,
                                                                int A, int B, float* dhd) {
  const int i = blockIdx.x * 256 + threadIdx.x, b = i >> 4, j = i & 15;
  if (b >= B) return;
  float* out = dhd + (size_t)b * SAC_XW;
  if (j >= A) {
    if (j >= 2 * A) out[j] = 0.0f;
    return;
  }
  const float c = expf(log_ent_coef[0]) / (float)B;
  const float raw = zh[(size_t)b * SAC_XW + A + j], ls = fminf(fmaxf(raw, SAC_LOG_STD_MIN), SAC_LOG_STD_MAX), ep = eps[(size_t)b * A + j];
  const float t = xc[(size_t)b * SAC_XW + O + j];
  const float da = dx[(size_t)b * SAC_XW + O + j] + dx[(size_t)(B + b) * SAC_XW + O + j];
  const float one = 1.0f - t * t;
  const float dg = da * one + c * ((2.0f * t) * one / (one + SAC_SQUASH_EPS));
  out[j] = dg;
  out[A + j] = (raw < SAC_LOG_STD_MIN || raw > SAC_LOG_STD_MAX) ? 0.0f : dg * (expf(ls) * ep) - c;
}

// Adam (torch's: eps added to sqrt(v_hat)) on a flat vector, and the Polyak update of a target vector of the same length with
// the NEW parameters: target = (1 - tau) target + tau p (two roundings, SB3's mul_ then add). target may be null.
__global__ __launch_bounds__(256) void sac_adam_kernel(float* params, const float* grad, float* m, float* v, long long n, float lr, float beta1, float beta2, float eps,
                                                       float c1, float c2, float* target, float one_minus_tau, float tau) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const float g = grad[p];
  const float mk = beta1 * m[p] + (1.0f - beta1) * g;
  const float vk = beta2 * v[p] + ((1.0f - beta2) * g) * g;
  m[p] = mk; v[p] = vk;
  const float pn = params[p] - lr * (mk / c1) / (sqrtf(vk / c2) + eps);
  params[p] = pn;
  if (target) target[p] = one_minus_tau * target[p] + tau * pn;
}

// the Polyak update alone
__global__ __launch_bounds__(256) void sac_polyak_kernel(const float* params, float* target, long long n, float one_minus_tau, float tau) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p < n) target[p] = one_minus_tau * target[p] + tau * params[p];
}

}  // namespace

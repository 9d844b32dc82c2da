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

// ------------------------------------------------------------------------------------------------------------- THE MEMBER AXIS
// A population of learners (tb_sac_*_members / tb_tqc_*_members) runs every kernel of the gradient step below with ONE more
// argument in a trailing pack that is empty or holds that one, as PolicyMembers and PpoMembers are passed: with the pack empty a
// kernel is what it was, argument list included. Members share the replay arrays and nothing else.
//   tile kernels   SacMembers: blockIdx.z enumerates (member, net), member = z / nets. Operands in the workspace (X, H, dZ, dX, Y)
//                  move by the member's workspace region `ws`, operands in a flat vector (W, bias, dW, db) by that vector's row
//                  stride `ps`. The tile's chain is the same chain: a member changes base addresses, never an order or an operand.
//   row kernels    SacRowMembers: the member is blockIdx.y (blockIdx.x in the one-workgroup reductions): its index row, its noise
//                  row, log_ent_coef[m], hp[m].gamma, its y row, its statistics row [4], ent_grad[m], its workspace region.
//   Adam / Polyak  SacAdamMembers: blockIdx.y; lr and tau from hp[m], 1 - tau formed as the host forms it for one learner.
// No kernel reads or writes between two members' rows: every offset inside a row is the single-member offset.
struct SacMembers { int nets; long long ws, ps; };  // floats
struct SacRowMembers {
  long long idx, eps, act, logp, y, ws;  // the rows' strides: idx in entries, the others in floats
  const TbSacMemberHp* hp;
};
struct SacAdamMembers { long long stride; const TbSacMemberHp* hp; int which_lr; };
template <class T> TB_DEV void sac_shift(T*& p, long long by) { if (p) p += by; }

// ---------------------------------------------------------------------------------------------------------------- tile kernels
struct SacFwdArgs {
  const float* x; int xs; long long xz;  // X[b][k] at x[z xz + b xs + k]
  const float* w; int wrs; long long wz; // W[o][k] at w[z wz + o wrs + k]
  const float* bias;                     // b[o] at bias[z wz + o]
  float* y; int ys; long long yz;        // Y[b][o] at y[z yz + b ys + o]
  int B, K, M;                           // rows, inputs, outputs
};

// grid (ceil(B / 64), ceil(M / 16), nets), 256 threads: wave w of block x takes rows 64 x + 16 w ..
template <bool RELU, class... MEMBERS>
__global__ __launch_bounds__(256) void sac_forward_kernel(SacFwdArgs a, MEMBERS... members) {
  static_assert(sizeof...(MEMBERS) <= 1, "no argument, or one SacMembers");
  int z = blockIdx.z;
  if constexpr (sizeof...(MEMBERS) != 0) {
    const SacMembers mb = (members, ...);
    const int m = z / mb.nets;
    z -= m * mb.nets;
    a.x += m * mb.ws; a.y += m * mb.ws; a.w += m * mb.ps; a.bias += m * mb.ps;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, e = lane & 15;
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
template <bool MASK, class... MEMBERS>
__global__ __launch_bounds__(256) void sac_backward_kernel(SacBwdArgs a, MEMBERS... members) {
  static_assert(sizeof...(MEMBERS) <= 1, "no argument, or one SacMembers");
  int z = blockIdx.z;
  if constexpr (sizeof...(MEMBERS) != 0) {
    const SacMembers mb = (members, ...);
    const int m = z / mb.nets;
    z -= m * mb.nets;
    a.dz += m * mb.ws; a.dx += m * mb.ws; a.w += m * mb.ps;
    if (MASK) a.h += m * mb.ws;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, e = lane & 15;
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
template <class... MEMBERS>
__global__ __launch_bounds__(256) void sac_wgrad_kernel(SacWgradArgs a, MEMBERS... members) {
  static_assert(sizeof...(MEMBERS) <= 1, "no argument, or one SacMembers");
  int z = blockIdx.z;
  if constexpr (sizeof...(MEMBERS) != 0) {
    const SacMembers mb = (members, ...);
    const int m = z / mb.nets;
    z -= m * mb.nets;
    a.dz += m * mb.ws; a.h += m * mb.ws; a.gw += m * mb.ps; a.gb += m * mb.ps;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, e = lane & 15;
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
template <class... MEMBERS>
__global__ __launch_bounds__(256) void sac_gather_kernel(const float* obs, int O, const float* act, int A, const long long* idx, long long n_rows, int B, float* out,
                                                         MEMBERS... members) {
  static_assert(sizeof...(MEMBERS) <= 1, "no argument, or one SacRowMembers");
  if constexpr (sizeof...(MEMBERS) != 0) {
    const SacRowMembers mb = (members, ...);
    idx += blockIdx.y * mb.idx; out += blockIdx.y * mb.ws;
  }
  const int i = blockIdx.x * 256 + threadIdx.x, b = i >> 4, c = i & 15;
  if (b >= B) return;
  const long long row = sac_row(idx, b, n_rows);
  float v = 0.0f;
  if (c < O) v = obs[(size_t)row * O + c];
  else if (act && c < O + A) v = act[(size_t)row * A + (c - O)];
  out[(size_t)b * SAC_XW + c] = v;
}

// the squashed sample of one action component from the head's outputs (ls: the clamped log_std): ONE copy for sac_sample_kernel and
// tb_sac_evaluate_kernel, so the two cannot drift
TB_DEV float sac_squash_sample(float mu, float log_std, float ep, float& ls) {
  ls = fminf(fmaxf(log_std, SAC_LOG_STD_MIN), SAC_LOG_STD_MAX);
  const float gs = mu + expf(ls) * ep;
  return tanhf(gs);
}

// one thread per row: the squashed sample and its log-probability from the head's outputs zh[b] = mu [A] | log_std [A];
// xc[b] = the row's observation | the sample | 0: the critics' input; lp[b][0] = logp. act_out / logp_out may be null
template <class... MEMBERS>
__global__ __launch_bounds__(256) void sac_sample_kernel(const float* x0, const float* zh, const float* eps, int O, int A, int B, float* act_out, float* logp_out, float* xc,
                                                         float* lp, MEMBERS... members) {
  static_assert(sizeof...(MEMBERS) <= 1, "no argument, or one SacRowMembers");
  if constexpr (sizeof...(MEMBERS) != 0) {
    const SacRowMembers mb = (members, ...);
    const long long m = blockIdx.y;
    x0 += m * mb.ws; zh += m * mb.ws; xc += m * mb.ws; lp += m * mb.ws; eps += m * mb.eps;
    sac_shift(act_out, m * mb.act); sac_shift(logp_out, m * mb.logp);
  }
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const float* z = zh + (size_t)b * SAC_XW;
  float* xr = xc + (size_t)b * SAC_XW;
  float s_gauss = 0.0f, s_squash = 0.0f;
  for (int c = 0; c < SAC_XW; ++c) xr[c] = c < O ? x0[(size_t)b * SAC_XW + c] : 0.0f;
  for (int j = 0; j < A; ++j) {
    const float ep = eps[(size_t)b * A + j];
    float ls;
    const float t = sac_squash_sample(z[j], z[A + j], ep, ls);
    s_gauss += (-0.5f * ep * ep - ls) - TB_LN_SQRT_2PI;
    s_squash += logf((1.0f - t * t) + SAC_SQUASH_EPS);
    xr[O + j] = t;
    if (act_out) act_out[(size_t)b * A + j] = t;
  }
  const float logp = s_gauss - s_squash;
  if (logp_out) logp_out[b] = logp;
  lp[(size_t)b * SAC_XW] = logp;
}

// what a member's target kernel reads and writes of its own (sac_target_kernel, tqc_target_kernel)
TB_DEV void sac_member_target(const SacRowMembers& mb, long long m, const long long*& idx, const float*& qt, const float*& logp_next, const float*& log_ent_coef, float& gamma,
                              float*& y) {
  idx += m * mb.idx; qt += m * mb.ws; logp_next += m * mb.ws; log_ent_coef += m; gamma = mb.hp[m].gamma; y += m * mb.y;
}
// ... and its actor-loss kernel (sac_actor_loss_kernel, tqc_actor_loss_kernel)
TB_DEV void sac_member_actor_loss(const SacRowMembers& mb, long long m, const float*& q, const float*& lp, const float*& log_ent_coef, float*& dq, float*& ent_grad,
                                  double*& stats) {
  q += m * mb.ws; lp += m * mb.ws; dq += m * mb.ws; log_ent_coef += m; ent_grad += m; stats += 4 * m;
}

// y = r + (1 - d) gamma (min(Q1t, Q2t) - alpha logp'); a terminal row is selected, not multiplied: y = r bit for bit
template <class... MEMBERS>
__global__ __launch_bounds__(256) void sac_target_kernel(const float* reward, const float* done, const long long* idx, long long n_rows, int B, const float* qt,
                                                         const float* logp_next, const float* log_ent_coef, float gamma, float* y, MEMBERS... members) {
  static_assert(sizeof...(MEMBERS) <= 1, "no argument, or one SacRowMembers");
  if constexpr (sizeof...(MEMBERS) != 0) sac_member_target((members, ...), blockIdx.y, idx, qt, logp_next, log_ent_coef, gamma, y);
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
template <class... MEMBERS>
__global__ __launch_bounds__(256) void sac_critic_loss_kernel(const float* q, const float* y, int B, float* dq, double* stats, MEMBERS... members) {
  static_assert(sizeof...(MEMBERS) <= 1, "no argument, or one SacRowMembers");
  if constexpr (sizeof...(MEMBERS) != 0) {  // one workgroup per member
    const SacRowMembers mb = (members, ...);
    const long long m = blockIdx.x;
    q += m * mb.ws; dq += m * mb.ws; y += m * mb.y; stats += 4 * m;
  }
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
template <class... MEMBERS>
__global__ __launch_bounds__(256) void sac_actor_loss_kernel(const float* q, const float* lp, const float* log_ent_coef, float target_entropy, int B, float* dq,
                                                             float* ent_grad, double* stats, MEMBERS... members) {
  static_assert(sizeof...(MEMBERS) <= 1, "no argument, or one SacRowMembers");
  if constexpr (sizeof...(MEMBERS) != 0) sac_member_actor_loss((members, ...), blockIdx.x, q, lp, log_ent_coef, dq, ent_grad, stats);  // one workgroup per member
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
template <class... MEMBERS>
__global__ __launch_bounds__(256) void sac_head_backward_kernel(const float* zh, const float* xc, const float* dx, const float* eps, const float* log_ent_coef, int O,
                                                                int A, int B, float* dhd, MEMBERS... members) {
  static_assert(sizeof...(MEMBERS) <= 1, "no argument, or one SacRowMembers");
  if constexpr (sizeof...(MEMBERS) != 0) {
    const SacRowMembers mb = (members, ...);
    const long long m = blockIdx.y;
    zh += m * mb.ws; xc += m * mb.ws; dx += m * mb.ws; dhd += m * mb.ws; eps += m * mb.eps; log_ent_coef += m;
  }
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

// a member's target row and its tau (sac_adam_kernel, sac_polyak_kernel); 1 - tau as tb_sac_adam's host code forms it
TB_DEV void sac_member_polyak(const SacAdamMembers& mb, long long k, float*& target, float& one_minus_tau, float& tau) {
  sac_shift(target, k * mb.stride);
  tau = mb.hp[k].tau;
  one_minus_tau = (float)(1.0 - (double)tau);
}

// Adam (torch's: eps added to sqrt(v_hat)) on a flat vector, and the Polyak update of a target vector of the same length with
// the NEW parameters: target = (1 - tau) target + tau p (two roundings, SB3's mul_ then add). target may be null.
template <class... MEMBERS>
__global__ __launch_bounds__(256) void sac_adam_kernel(float* params, const float* grad, float* m, float* v, long long n, float lr, float beta1, float beta2, float eps,
                                                       float c1, float c2, float* target, float one_minus_tau, float tau, MEMBERS... members) {
  static_assert(sizeof...(MEMBERS) <= 1, "no argument, or one SacAdamMembers");
  if constexpr (sizeof...(MEMBERS) != 0) {
    const SacAdamMembers mb = (members, ...);
    const long long k = blockIdx.y, by = k * mb.stride;
    params += by; grad += by; m += by; v += by;
    lr = mb.which_lr == 0 ? mb.hp[k].lr_actor : mb.which_lr == 1 ? mb.hp[k].lr_critic : mb.hp[k].lr_ent;
    sac_member_polyak(mb, k, target, one_minus_tau, tau);
  }
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
template <class... MEMBERS>
__global__ __launch_bounds__(256) void sac_polyak_kernel(const float* params, float* target, long long n, float one_minus_tau, float tau, MEMBERS... members) {
  static_assert(sizeof...(MEMBERS) <= 1, "no argument, or one SacAdamMembers");
  if constexpr (sizeof...(MEMBERS) != 0) {
    const SacAdamMembers mb = (members, ...);
    params += blockIdx.y * mb.stride;
    sac_member_polyak(mb, blockIdx.y, target, one_minus_tau, tau);
  }
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p < n) target[p] = one_minus_tau * target[p] + tau * params[p];
}

// ------------------------------------------------------------------------------- whole episodes in one launch (tb_sac_evaluate)
// The whole-episode env wave (tb_kernels.hpp) with SAC's / TQC's 256-wide actor inside the episode loop. A workgroup owns 16 envs and is
// FOUR waves, one per SIMD (__launch_bounds__(256): the env wave keeps the register budget it has in tb_policy_evaluate_kernel).
// Waves 0-3 share the actor; wave 3 is also the env wave: the 16 envs' state in its registers, lanes >= 16 and lanes whose episode
// is over step the dummy (idle_env). The actor does not fit registers or LDS (283 KB): its weights stream from global memory (L2)
// every step, straight from the flat TB_SAC_ACTOR vector, and the activations of the 16 rows live in LDS.
// ARITHMETIC: every output element is sac_forward_kernel's: one f32-input MFMA chain from a zero accumulator over k ascending in
// steps of four (zeros beyond O in the first layer), then + bias, then fmaxf(., 0) on the hidden layers. An output row depends on
// its own input row only and a tile on its own chain only, so which wave runs which tile changes no bit. A wave owns 4 of the 16
// tiles of a hidden layer (four interleaved chains hide the MFMA's dependent latency); mu is one tile on wave 0, log_std on wave 1.
// LDS: s_obs [16][O]; s_h1, s_h2 [16][SAC_EV_STRIDE]: a row stride of 260 floats puts the 16 rows x 4 k's a lane group reads of
// one MFMA step into 64 different banks (4 e + g; 256 would be a 16-way conflict) and keeps the float4 stores aligned; s_head
// [16][16]: mu at [0 .. A), log_std at [8 .. 8 + A); s_go.
// BARRIERS. Every wave executes one barrier behind the set-up and FOUR per iteration, on every path; no wave returns inside the
// loop, and the loop ends at T_MAX whatever s_go holds:
//   set-up  env wave: s_obs = the reset observations (idle rows too); all: the outline table          -> barrier 0
//   (1)     all: s_h1 = relu(W0 s_obs + b0), tiles 4 w .. 4 w + 3                                      -> barrier 1  "h1 is in LDS"
//   (2)     all: s_h2 = relu(W1 s_h1 + b1)                                                             -> barrier 2  "h2 is in LDS"
//   (3)     wave 0: s_head mu, wave 1: s_head log_std (from s_h2); env wave: draws the noise           -> barrier 3  "the head is in LDS"
//   (4)     env wave: sample (s_head), trace (s_obs), env step, s_obs of the live envs, lane 0: s_go   -> barrier 4  "obs and s_go are in LDS"
//           all: leave unless loop_goes_on (tb_kernels.hpp, with the proof that every wave reaches the same verdict; the env wave's
//           vote_go is in (4), the barrier that guards the next vote is barrier 3 of t + 1).
// Who may overwrite what: s_h1 is next written in (1) of t + 1, behind barrier 4, its readers ((2) of t) are in front of barrier
// 2; s_h2 is next written behind barrier 1 of t + 1, its readers ((3) of t) are in front of barrier 3; s_head is next written
// behind barrier 2 of t + 1, its reader ((4) of t) is in front of barrier 4; s_obs and s_go are written behind barrier 3 only,
// s_obs is read in front of barrier 1 (and by the env wave itself in (4), before it writes), s_go between barrier 4 and barrier 1.
constexpr int SAC_EV_STRIDE = SAC_H + 4;

struct SacEvalArgs {
  const float* actor;  // the flat TB_SAC_ACTOR vector
  double* ret;         // [n] (SwingRacket: without the terminal reward, which tb_es_fold_kernel adds)
  int32_t* len;        // [n]
  // optional trace, rows [t][n] (TbSacEvalTrace); t_max = 0: off
  int t_max;
  float *t_obs, *t_eps, *t_act, *t_rew;
  uint8_t* t_done;
};

// NT tiles of one layer for the 16 rows x (LDS): tile j's weight row of this lane is w + j * tile_step. acc[j][r]: output
// 16 j + 4 g + r of row e. The chain of sac_forward_kernel per tile: whole chunks of SAC_UNROLL steps, then single steps.
template <int NT, int K>
TB_DEV void sac_ev_chain(const float* w, int tile_step, bool o_in, const float* xrow, int g, f32x4* acc) {
#pragma unroll
  for (int j = 0; j < NT; ++j) acc[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  constexpr int KW = K / (4 * SAC_UNROLL) * (4 * SAC_UNROLL);
#pragma unroll 1  // (one chunk's loads in flight, not the layer's: the env wave's state stays in registers beside them)
  for (int k0 = 0; k0 < KW; k0 += 4 * SAC_UNROLL) {
    float wl[NT][SAC_UNROLL], xl[SAC_UNROLL];
#pragma unroll
    for (int u = 0; u < SAC_UNROLL; ++u) {
      xl[u] = xrow[k0 + 4 * u + g];
#pragma unroll
      for (int j = 0; j < NT; ++j) wl[j][u] = w[j * tile_step + k0 + 4 * u + g];
    }
#pragma unroll
    for (int u = 0; u < SAC_UNROLL; ++u) {
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(o_in ? wl[j][u] : 0.0f, xl[u], acc[j], 0, 0, 0);
    }
  }
#pragma unroll
  for (int k0 = KW; k0 < K; k0 += 4) {
    const int k = k0 + g, kc = k < K ? k : K - 1;  // (every address is a valid one; what lies outside is selected away)
    const bool k_in = k < K;
    const float xl = xrow[kc];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const float wl = w[j * tile_step + kc];
      acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32((o_in && k_in) ? wl : 0.0f, k_in ? xl : 0.0f, acc[j], 0, 0, 0);
    }
  }
}

// one hidden layer's share of a wave: h[e][64 wave + 16 j + 4 g + r] = relu(acc + bias)
template <int K>
TB_DEV void sac_ev_hidden(const float* W, const float* bias, const float* x, int xs, float* h, int wave, int g, int e) {
  f32x4 acc[4];
  const int o0 = 64 * wave;
  sac_ev_chain<4, K>(W + (size_t)(o0 + e) * K, 16 * K, true, x + e * xs, g, acc);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int oo = o0 + 16 * j + 4 * g;
    float4 v;
    v.x = fmaxf(acc[j][0] + bias[oo], 0.0f); v.y = fmaxf(acc[j][1] + bias[oo + 1], 0.0f);
    v.z = fmaxf(acc[j][2] + bias[oo + 2], 0.0f); v.w = fmaxf(acc[j][3] + bias[oo + 3], 0.0f);
    *reinterpret_cast<float4*>(h + e * SAC_EV_STRIDE + oo) = v;
  }
}

// The actor's stages (1)-(3) of one step, for the 16 observation rows in s_obs: ONE copy for tb_sac_evaluate_kernel and
// tb_sac_collect_kernel. Every wave of the workgroup calls it; barriers 1 and 2 are inside, and the caller places barrier 3 ("the head
// is in LDS") behind it -- the env wave draws its noise in between, while waves 0 and 1 run the head.
template <int KIND>
TB_DEV void sac_actor_stage(const float* actor, const float* s_obs, float* s_h1, float* s_h2, float* s_head, int wave, int g, int er) {
  using L = SacLayout<KIND>;
  constexpr int NA = Dims<KIND>::A, NO = Dims<KIND>::O;
  sac_ev_hidden<NO>(actor + L::PI_W0, actor + L::PI_B0, s_obs, NO, s_h1, wave, g, er);
  __syncthreads();  // barrier 1: h1 is in LDS
  sac_ev_hidden<SAC_H>(actor + L::PI_W1, actor + L::PI_B1, s_h1, SAC_EV_STRIDE, s_h2, wave, g, er);
  __syncthreads();  // barrier 2: h2 is in LDS
  if (wave < 2) {  // mu (wave 0) and log_std (wave 1): one tile each, rows er < A of the head's block
    const float* hw = actor + L::PI_HEAD + wave * L::PI_HEAD_BLOCK;
    const bool o_in = er < NA;
    f32x4 acc[1];
    sac_ev_chain<1, SAC_H>(hw + (size_t)(o_in ? er : 0) * SAC_H, 0, o_in, s_h2 + er * SAC_EV_STRIDE, g, acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int oo = 4 * g + r;
      if (oo < NA) s_head[er * 16 + wave * 8 + oo] = acc[0][r] + hw[NA * SAC_H + oo];
    }
  }
}

// THE MEMBERS FORM (tb_sac_evaluate_members: a population of actors, one launch) is this kernel with ONE more argument, a
// PolicyMembers (tb_kernels.hpp), as tb_policy_evaluate_kernel has it: S.actor then holds the members' flat vectors `stride` floats
// apart, env i is member i / per_member's, and per_member is a multiple of TB_POLICY_SLICE (the host refuses anything else), so the
// 16 envs of a workgroup -- the 16 rows of every MFMA tile of its four waves -- share ONE member. member_blob_offset is a function of
// blockIdx.x and two kernel arguments alone: the vector's address stays in scalar registers like S.actor itself. Every weight address
// is S.actor + a layout offset below the vector's length, so floats between two members' vectors are never read. The actor stage,
// the barriers, the vote and the exit are the same lines. The argument is a trailing pack, empty or one PolicyMembers, so that
// tb_sac_evaluate_kernel<KIND, RG> remains the kernel it was, argument list included.
template <int KIND, bool RG, typename... MEMBERS>
__global__ void __launch_bounds__(256) tb_sac_evaluate_kernel(KArgs A, SacEvalArgs S, MEMBERS... members) {
  static_assert(sizeof...(MEMBERS) <= 1, "no argument, or one PolicyMembers");
  if constexpr (sizeof...(MEMBERS) != 0) S.actor += member_blob_offset(members...);
  using L = SacLayout<KIND>;
  constexpr int NA = Dims<KIND>::A, NO = Dims<KIND>::O, E = TB_POLICY_SLICE, ENV_WAVE = 3;
  static_assert(NA == L::A && NO == L::O && E == 16 && NA <= 8, "the actor's rows are the envs of one slice");
  constexpr int T_MAX = episode_cap(KIND);
  __shared__ float4 s_hull[TB_HULL_LDS];
  __shared__ __attribute__((aligned(16))) float s_obs[E * NO];
  __shared__ __attribute__((aligned(16))) float s_h1[E * SAC_EV_STRIDE];
  __shared__ __attribute__((aligned(16))) float s_h2[E * SAC_EV_STRIDE];
  __shared__ __attribute__((aligned(16))) float s_head[E * 16];
  __shared__ int s_go;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, g = lane >> 4, er = lane & 15;
  const bool env_wave = wave == ENV_WAVE;
  stage_hull(s_hull, A.hull, A.P.n_hull);
  const int i = blockIdx.x * E + lane;
  const bool live = env_wave && lane < E && i < A.n;
  EnvRegs e;
  Manifold M;
  enter_env_wave<KIND>(A, i, live, lane, !policy_rollout_rows_in_registers(KIND), e, M);  // the state tb_reset just wrote: the episode's start, no contacts cached
  uint32_t cnt[TB_N_COUNTERS] = {};
  if (env_wave && lane < E) {  // (rows without an env hold the dummy's observation: finite, and no row reads another)
    float o[NO];
    make_obs<KIND>(e, o);
    publish_obs<NO>(s_obs, lane, o);
  }
  __syncthreads();  // barrier 0: the outline table and the episodes' first observations are in LDS
  KParams Pl = A.P;
  pin_substep_params(Pl);
  EpisodeTally ep = {live, 0.0, 0};
  constexpr unsigned FORM = loop_step_form(RG, true, policy_rollout_rows_in_registers(KIND));
  TB_DIAG_STAMPS_BEGIN(st);
  for (int t = 0;; ++t) {
    sac_actor_stage<KIND>(S.actor, s_obs, s_h1, s_h2, s_head, wave, g, er);
    float eps[NA];
#pragma unroll
    for (int k = 0; k < NA; ++k) eps[k] = 0.0f;
    if (env_wave && ep.active) policy_draw<KIND>(A, i, e, eps);  // while the head runs
    __syncthreads();  // barrier 3: the head is in LDS
    if (env_wave) {
      float a[NA], o[NO];
#pragma unroll
      for (int k = 0; k < NA; ++k) a[k] = 0.0f;
      const bool rec = ep.active && t < S.t_max;
      if (ep.active) {
#pragma unroll
        for (int k = 0; k < NA; ++k) {
          float ls;
          a[k] = sac_squash_sample(s_head[lane * 16 + k], s_head[lane * 16 + 8 + k], eps[k], ls);
        }
        if (rec) {
          const size_t row = (size_t)t * A.n + i;
#pragma unroll
          for (int k = 0; k < NO; ++k) S.t_obs[row * NO + k] = s_obs[lane * NO + k];
#pragma unroll
          for (int k = 0; k < NA; ++k) { S.t_eps[row * NA + k] = eps[k]; S.t_act[row * NA + k] = a[k]; }
        }
      }
      int ns = 1;
      bool d = false, parked = false;
      float rew = env_wave_step<KIND, FORM>(Pl, s_hull, e, M, a, o, ns, d, parked, cnt TB_STAMP_PASS);
      if (ep.active) {
        end_agent_step<KIND, RG, false>(A, i, e, M, parked, ns, (size_t)i, o, d, cnt);  // (tb_sac_evaluate claims a slot for every env)
        rew = tally_step(ep, t, rew, parked, d, e, M, cnt);
        if (rec) {
          S.t_rew[(size_t)t * A.n + i] = rew;
          S.t_done[(size_t)t * A.n + i] = d ? 1 : 0;
        }
        if (!d) publish_obs<NO>(s_obs, lane, o);
      }
      vote_go(s_go, lane, ep.active);
    }
    __syncthreads();  // barrier 4: the observations after step t, and s_go, are in LDS
    if (!loop_goes_on(s_go, t, T_MAX)) break;
  }
  if (live) { S.ret[i] = ep.ret; S.len[i] = ep.len; }
  if (env_wave) flush_counters(A.counters, cnt);
  TB_DIAG_STAMPS_END(st);
}

// ------------------------------------------------------------------------------- transitions into the replay ring (tb_sac_collect)
// n_steps agent steps of every env from the state the handle holds, ONE launch, every transition written as the replay ring stores
// it: tb_sac_evaluate_kernel's workgroup (16 envs, four waves, sac_actor_stage) around tb_policy_rollout_kernel<KIND, 1>'s env wave
// (state and contact cache in, in-loop restart_episode on done, SwingRacket parking at a launch's last step, state and cache out).
// Rows [t][n]: obs = what step t acted on, action, reward, done (0.0f / 1.0f), next_obs = what tb_step would have returned (a done
// row: the next episode's first observation), eps (optional). The trip count is the argument n_steps for every wave: no s_go, no
// early exit. UNIFORM (a kernel argument, the same in every wave of the grid): no actor stage runs -- barriers 1 and 2 are skipped by
// every wave alike -- and the action is policy_uniform's of the key policy_draw would have used.
// BARRIERS. One behind the set-up, then FOUR per iteration in actor mode and TWO in uniform mode, on every path; no wave returns
// inside the loop:
//   set-up  env wave: s_obs = the observations of the loaded state (idle rows too); all: the outline table -> barrier 0
//   (1)     all: s_h1 = relu(W0 s_obs + b0)            [actor mode]                                       -> barrier 1  "h1 is in LDS"
//   (2)     all: s_h2 = relu(W1 s_h1 + b1)             [actor mode]                                       -> barrier 2  "h2 is in LDS"
//   (3)     wave 0: s_head mu, wave 1: s_head log_std  [actor mode]; env wave: draws noise / the action   -> barrier 3  "the head is in LDS"
//   (4)     env wave: sample (s_head), the obs row (s_obs), env step, restart on done, s_obs = next obs   -> barrier 4  "obs is in LDS"
//           env wave: the step's other rows go to memory behind barrier 4, while the actor already runs step t + 1
// Who may overwrite what: s_h1 is next written in (1) of t + 1, behind barrier 4, its readers ((2) of t) are in front of barrier 2;
// s_h2 is next written behind barrier 1 of t + 1, its readers ((3) of t) are in front of barrier 3; s_head is next written behind
// barrier 2 of t + 1, its reader ((4) of t) is in front of barrier 4; s_obs is written behind barrier 3 only (by the env wave, after
// its own read of the row) and read by the others in front of barrier 1. Uniform mode touches s_obs only, in the env wave.
struct SacCollectArgs {
  const float* actor;  // the flat TB_SAC_ACTOR vector (null in uniform mode)
  int n_steps, uniform;
  float *obs, *next_obs, *action, *reward, *done, *eps;  // TbSacCollectOut's rows [n_steps][n]; eps may be null
};

template <int KIND, bool RG>
__global__ void __launch_bounds__(256) tb_sac_collect_kernel(KArgs A, SacCollectArgs S) {
  using L = SacLayout<KIND>;
  constexpr int NA = Dims<KIND>::A, NO = Dims<KIND>::O, E = TB_POLICY_SLICE, ENV_WAVE = 3;
  static_assert(NA == L::A && NO == L::O && E == 16 && NA <= 8, "the actor's rows are the envs of one slice");
  __shared__ float4 s_hull[TB_HULL_LDS];
  __shared__ __attribute__((aligned(16))) float s_obs[E * NO];
  __shared__ __attribute__((aligned(16))) float s_h1[E * SAC_EV_STRIDE];
  __shared__ __attribute__((aligned(16))) float s_h2[E * SAC_EV_STRIDE];
  __shared__ __attribute__((aligned(16))) float s_head[E * 16];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, g = lane >> 4, er = lane & 15;
  const bool env_wave = wave == ENV_WAVE;
  const bool uniform = S.uniform != 0;  // (a kernel argument: the same verdict in every wave of the grid)
  stage_hull(s_hull, A.hull, A.P.n_hull);
  const int i = blockIdx.x * E + lane;
  const bool live = env_wave && lane < E && i < A.n;
  EnvRegs e;
  Manifold M;
  enter_env_wave<KIND>(A, i, live, lane, !policy_rollout_rows_in_registers(KIND), e, M);
  const bool had_contacts = load_contacts<RG>(A, i, live, M);
  uint32_t cnt[TB_N_COUNTERS] = {};
  bool any_reset = false;
  if (env_wave && lane < E) {  // (rows without an env hold the dummy's observation: finite, and no row reads another)
    float o[NO];
    make_obs<KIND>(e, o);  // what the step that left this state returned (tennis_step / end_agent_step / restart_episode: make_obs all)
    publish_obs<NO>(s_obs, lane, o);
  }
  __syncthreads();  // barrier 0: the outline table and the observations the first step acts on are in LDS
  KParams Pl = A.P;
  pin_substep_params(Pl);
  constexpr unsigned FORM = loop_step_form(RG, true, policy_rollout_rows_in_registers(KIND));
  TB_DIAG_STAMPS_BEGIN(st);
  for (int t = 0; t < S.n_steps; ++t) {
    if (!uniform) sac_actor_stage<KIND>(S.actor, s_obs, s_h1, s_h2, s_head, wave, g, er);
    float eps[NA], a[NA];
#pragma unroll
    for (int k = 0; k < NA; ++k) { eps[k] = 0.0f; a[k] = 0.0f; }
    if (live) {  // while the head runs
      if (uniform) policy_uniform<NA>(A.pol_seed, A.env_id_base + (unsigned long long)i, e.episode, e.step_count, a);
      else policy_draw<KIND>(A, i, e, eps);
    }
    __syncthreads();  // barrier 3: the head is in LDS
    float o[NO], rew = 0.0f;
    bool d = false;
    const size_t row = (size_t)t * A.n + i;
    if (env_wave) {
      if (live) {
        if (!uniform) {
#pragma unroll
          for (int k = 0; k < NA; ++k) {
            float ls;
            a[k] = sac_squash_sample(s_head[lane * 16 + k], s_head[lane * 16 + 8 + k], eps[k], ls);
          }
        }
        float oi[NO];
#pragma unroll
        for (int k = 0; k < NO; ++k) oi[k] = s_obs[lane * NO + k];
        write_obs<KIND>(S.obs, row, oi);
      }
      int ns = 1;
      bool parked = false;
      rew = env_wave_step<KIND, FORM>(Pl, s_hull, e, M, a, o, ns, d, parked, cnt TB_STAMP_PASS);
      if (live) {
        end_agent_step<KIND, RG, true>(A, i, e, M, parked, ns, row, o, d, cnt);  // (a parked step's reward: the fast-forward's, into S.reward[row])
        if (d) restart_on_done<KIND>(A, s_hull, i, e, M, o, cnt, any_reset);
        publish_obs<NO>(s_obs, lane, o);
      }
    }
    __syncthreads();  // barrier 4: the observations step t + 1 acts on are in LDS
    if (live) {
      store_row2<NA>(S.action, row, a);
      if (S.eps) store_row2<NA>(S.eps, row, eps);
      write_obs<KIND>(S.next_obs, row, o);
      S.reward[row] = rew;
      S.done[row] = d ? 1.0f : 0.0f;
    }
  }
  if (live) save_env<KIND, RG>(A, i, e, M, any_reset, had_contacts);
  if (env_wave) flush_counters(A.counters, cnt);
  TB_DIAG_STAMPS_END(st);
}

}  // namespace

// The TQC learner's kernels (C ABI tb_tqc_* in include/tb_stepper.h; tennisbot_rl_amd/tqc.py is the caller). Device code only;
// included by tb_stepper.hip after tb_sac.hpp, whose tile kernels, gather, sample, head backward, Adam and Polyak kernels it uses
// as they are: TQC's actor is SAC's, and its critics differ from SAC's in the last layer alone, which has 25 outputs (the
// quantiles) instead of one. A head is one launch of a tile kernel with K = 256, M = 25: two column tiles, the second of 9 live
// columns, and in the backward kernel a reduction of 6 whole k-steps and one of a single live row. The host path is SAC's as
// well: tb_stepper.hip writes each stage once, and its descriptor TqcAlgo supplies this file's layouts (TqcLayout, TqcWs), the
// head's 25 outputs in rows of 32, and the launches of the three loss kernels below.
//
// What is TQC's own is row-wise, one wave per batch row, no LDS and no barrier in the per-row work:
//   tqc_target_kernel       the 50 target quantiles of a row, sorted by rank counting, the 46 smallest into y[b][0 .. 46)
//   tqc_critic_loss_kernel  the quantile Huber loss over the 2 x 25 x 46 pairs of a row and its gradient for the 50 head outputs
//   tqc_loss_sum_kernel     the batch's loss from the rows' sums: one workgroup, sac_block_sum's tree
//   tqc_actor_loss_kernel   the actor loss's scalars and the constant gradient -1 / (50 B) of the mean over quantiles and critics
// The head regions of the workspace are [2][B][32]: 25 live columns, 7 of padding that the loss kernels keep at zero. Losses and
// statistics are float64 sums in one fixed order; no float atomics; every loop is bounded by its arguments.
#pragma once

namespace {

constexpr int TQC_Q = TB_TQC_QUANTILES;  // quantiles per critic
constexpr int TQC_N = 2 * TQC_Q;         // a row's target quantiles before truncation, and its head outputs
constexpr int TQC_KEEP = TB_TQC_TARGETS; // what is left after dropping the top 2 per net
constexpr int TQC_HW = 32;               // padded width of a head row in the workspace
static_assert(TQC_KEEP == TQC_N - 2 * TB_TQC_DROP_PER_NET && TQC_N <= 64 && TQC_Q <= TQC_HW, "one wave holds a row's quantiles");

template <int KIND> struct TqcLayout {
  using S = SacLayout<KIND>;
  // one critic: W0 [256][O + A] b0 | W1 b1 | W2 [25][256] b2; the flat vector holds qf0 then qf1. The actor is SacLayout's.
  static constexpr int Q_W2 = S::Q_B1 + SAC_H, Q_B2 = Q_W2 + TQC_Q * SAC_H, Q_ONE = Q_B2 + TQC_Q, Q_P = 2 * Q_ONE;
};
static_assert(TqcLayout<TB_ENV_SWING>::Q_P == 151090 && TqcLayout<TB_ENV_TENNIS>::Q_P == 152114, "critic parameter count");

// The workspace: SAC's layout with head regions (QT, Q, DQ) of [2][B][32], and one double per row for the critic loss (RL)
using TqcWs = SacWsT<TQC_HW, 2>;
static_assert(TqcWs::QT == 2176 && TqcWs::Q == 3280 && TqcWs::DQ == 3344 && TqcWs::DX == 4432 && TqcWs::PER_ROW == 4994, "TQC's workspace layout");
static_assert(TqcWs::RL % 2 == 0, "the row sums are 8-byte aligned");

// one wave per row, four rows per workgroup: grid ceil(B / 4), 256 threads. Lane l < 50 holds quantile l % 25 of target net
// l / 25; its rank is the number of lanes that precede it in the total order (is-NaN, value, lane), so equal values take
// consecutive slots and a NaN sorts last, as torch.sort does. The other lanes' values come from v_readlane, lane by lane.
// y[b][rank] = r + gamma (z - alpha logp') for rank < 46; a terminal row is selected, not multiplied: y = r bit for bit.
template <class... MEMBERS>
__global__ __launch_bounds__(256) void tqc_target_kernel(const float* reward, const float* done, const long long* idx, long long n_rows, int B, const float* qt,
                                                         const float* logp_next, const float* log_ent_coef, float gamma, float* y, MEMBERS... members) {
  static_assert(sizeof...(MEMBERS) <= 1, "no argument, or one SacRowMembers (tb_sac.hpp, THE MEMBER AXIS)");
  if constexpr (sizeof...(MEMBERS) != 0) sac_member_target((members, ...), blockIdx.y, idx, qt, logp_next, log_ent_coef, gamma, y);
  const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const bool live = lane < TQC_N;
  const int l = live ? lane : 0, n = l / TQC_Q, i = l - n * TQC_Q;
  const float v = qt[(size_t)(n * (long long)B + b) * TQC_HW + i];
  const bool v_nan = v != v;
  int rank = 0;
#pragma unroll 10  // (all 50 at once would hold 50 SGPRs of lane values and spill)
  for (int m = 0; m < TQC_N; ++m) {
    const float u = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), m));
    const bool u_nan = u != u;
    const bool before = u_nan != v_nan ? v_nan : u_nan ? m < lane : (u < v || (u == v && m < lane));
    rank += before ? 1 : 0;
  }
  const long long row = sac_row(idx, b, n_rows);
  const float alpha = expf(log_ent_coef[0]), r = reward[row];
  const float out = done[row] != 0.0f ? r : r + gamma * (v - alpha * logp_next[(size_t)b * SAC_XW]);
  if (live && rank < TQC_KEEP) y[(size_t)b * TQC_KEEP + rank] = out;
}

// one wave per row, four rows per workgroup: grid ceil(B / 4), 256 threads. Lane l < 50 owns theta = Q_n(s, a)[i], n = l / 25,
// i = l % 25, tau_i = (i + 0.5) / 25, and runs j = 0 .. 45 in index order over the row's targets, delta = y[b][j] - theta:
//   loss term |tau_i - [delta < 0]| H(delta), H = |delta| - 0.5 if |delta| > 1 else delta^2 / 2
//   dq[n][b][i] = -(1 / (B 2300)) sum_j |tau_i - [delta < 0]| clamp(delta, -1, 1)
// Lanes 50 .. 63 write the zeros of columns 25 .. 31 of both nets' rows. row_loss[b] = the row's 2300 terms: float64, the
// lane's sum in j order, then the wave's xor tree.
template <class... MEMBERS>
__global__ __launch_bounds__(256) void tqc_critic_loss_kernel(const float* q, const float* y, int B, float* dq, double* row_loss, MEMBERS... members) {
  static_assert(sizeof...(MEMBERS) <= 1, "no argument, or one SacRowMembers");
  if constexpr (sizeof...(MEMBERS) != 0) {  // (row_loss lies in the member's workspace region, whose stride is a multiple of 8 bytes)
    const SacRowMembers mb = (members, ...);
    const long long m = blockIdx.y;
    q += m * mb.ws; dq += m * mb.ws; row_loss += m * (mb.ws / 2); y += m * mb.y;
  }
  const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const bool live = lane < TQC_N;
  const int pad = lane - TQC_N;                                                     // 0 .. 13 on the padding's lanes
  const int n = live ? lane / TQC_Q : pad / (TQC_HW - TQC_Q), i = live ? lane % TQC_Q : TQC_Q + pad % (TQC_HW - TQC_Q);
  const size_t at = (size_t)(n * (long long)B + b) * TQC_HW + i;
  const float theta = q[at], tau = ((float)i + 0.5f) / (float)TQC_Q;
  const float* yrow = y + (size_t)b * TQC_KEEP;
  float g = 0.0f;
  double part = 0.0;
  for (int j = 0; j < TQC_KEEP; ++j) {
    const float delta = yrow[j] - theta, ad = fabsf(delta);
    const float w = delta < 0.0f ? 1.0f - tau : tau;
    g += w * fminf(fmaxf(delta, -1.0f), 1.0f);
    part += (double)(w * (ad > 1.0f ? ad - 0.5f : (0.5f * delta) * delta));
  }
  dq[at] = live ? -g / ((float)B * (float)(TQC_N * TQC_KEEP)) : 0.0f;
  if (!live) part = 0.0;
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) part += __shfl_xor(part, w);
  if (lane == 0) row_loss[b] = part;
}

// stats[0] = the mean of the B 2300 loss terms from the rows' sums. One workgroup.
template <class... MEMBERS>
__global__ __launch_bounds__(256) void tqc_loss_sum_kernel(const double* row_loss, int B, double* stats, MEMBERS... members) {
  static_assert(sizeof...(MEMBERS) <= 1, "no argument, or one SacRowMembers");
  if constexpr (sizeof...(MEMBERS) != 0) {  // one workgroup per member
    const SacRowMembers mb = (members, ...);
    row_loss += blockIdx.x * (mb.ws / 2); stats += 4 * blockIdx.x;
  }
  __shared__ double s[256];
  double v = 0.0;
  for (int b = threadIdx.x; b < B; b += 256) v += row_loss[b];
  const double total = sac_block_sum(v, s);
  if (threadIdx.x == 0) stats[0] = total / ((double)B * (double)(TQC_N * TQC_KEEP));
}

// the actor loss mean_b(alpha logp - Qbar(s, a~)), Qbar the mean over a row's 50 head outputs (qf0's 25 in index order, then
// qf1's): dq = -1 / (50 B) in the 25 live columns of both nets' rows, 0 in the padding; stats[1] = the loss, stats[2] = mean
// logp, stats[3] = the gradient of log_ent_coef, -mean(logp + target_entropy), also written as float32 to ent_grad. One workgroup.
template <class... MEMBERS>
__global__ __launch_bounds__(256) void tqc_actor_loss_kernel(const float* q, const float* lp, const float* log_ent_coef, float target_entropy, int B, float* dq,
                                                             float* ent_grad, double* stats, MEMBERS... members) {
  static_assert(sizeof...(MEMBERS) <= 1, "no argument, or one SacRowMembers");
  if constexpr (sizeof...(MEMBERS) != 0) sac_member_actor_loss((members, ...), blockIdx.x, q, lp, log_ent_coef, dq, ent_grad, stats);  // one workgroup per member
  __shared__ double s[256];
  const float alpha = expf(log_ent_coef[0]), each = -1.0f / ((float)TQC_N * (float)B);
  double sl = 0.0, sp = 0.0, se = 0.0;
  for (int b = threadIdx.x; b < B; b += 256) {
    double qs = 0.0;
    for (int n = 0; n < 2; ++n) {
      const size_t at = (size_t)(n * (long long)B + b) * TQC_HW;
      for (int i = 0; i < TQC_HW; ++i) {
        if (i < TQC_Q) qs += (double)q[at + i];
        dq[at + i] = i < TQC_Q ? each : 0.0f;
      }
    }
    const float logp = lp[(size_t)b * SAC_XW];
    sl += (double)(alpha * logp) - qs / (double)TQC_N;
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

}  // namespace

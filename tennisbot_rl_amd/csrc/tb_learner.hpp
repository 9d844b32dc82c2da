// The PPO learner on the device (tb_ppo_gae, tb_ppo_grad, tb_ppo_apply): GAE, one minibatch's gradient, norm clip + Adam.
// Device code only; included by tb_stepper.hip after tb_kernels.hpp (Dims, PolicyNet, fast_tanh, f32x4 of tb_policy.hpp).
//
// Parameters travel as ONE flat fp32 vector in the order of build_actor_critic(...).named_parameters(), every tensor
// row-major as torch holds it (nn.Linear.weight is [out][in]):
//     log_std [A] | policy_net: W0 b0 W1 b1 (W2 b2) | value_net_body: the same | action_net W b | value_net W b
// (PpoLayout). The gradient, both Adam moments and every partial gradient use the same order.
//
// tb_ppo_grad_kernel. A workgroup of four waves takes TB_PPO_SHARE = 256 consecutive entries of the minibatch's index vector;
// wave w runs ONE tower (w >> 1: 0 = pi, 1 = vf; the two towers share nothing but the observation) over one half (w & 1) of
// them, 16 rows per tile, and never talks to the other waves: no barrier, no atomics. Per tile, on v_mfma_f32_16x16x4_f32 with
// the fragment conventions of tb_policy.hpp (everything transposed: features on the M axis, the 16 rows on N):
//   forward    Z^T[out][row]  = W[out][k] H^T[k][row]        A = weight fragment, B = the previous layer's C/D registers
//   backward   dH^T[in][row]  = W^T[in][out] dZ^T[out][row]   A = transposed weight fragment, B = dZ's C/D registers
//   weights    dW[out][in]   += dZ^T[out][row] H[row][in]     K = the rows: both operands need the row index on the lane
//                                                             GROUP, not on the lane -- one 16 x 16 transpose each through
//                                                             LDS (ppo_transpose: wave-private, no workgroup barrier)
// Forward and transposed weight fragments and every dW / db / d log_std accumulator stay in registers over the wave's whole
// share (128 rows: an fp32 chain of 128 per element at the most); at the end each wave writes its tower's slots of partial
// vector 2 * workgroup + half. tb_ppo_reduce_kernel then adds the partials per parameter in float64 in a fixed order.
// The minibatch's advantage mean / unbiased std come from tb_ppo_adv_stats_kernel (float64 sums of x and x^2 in 64 blocks,
// combined in a fixed order by every wave that needs them).
#pragma once

namespace {

constexpr int TB_PPO_SHARE = 256;       // rows of the index vector per workgroup
constexpr int TB_PPO_HALF = TB_PPO_SHARE / 2;
constexpr int TB_PPO_STAT_BLOCKS = 64;  // partial sums of the advantage statistics
constexpr float TB_LN_SQRT_2PI = 0.9189385332046727f;

template <int KIND, int NET = TB_NET_DEFAULT> struct PpoLayout {
  using N = PolicyNet<KIND, NET>;
  static constexpr int O = Dims<KIND>::O, A = Dims<KIND>::A, NH = N::NH, LAST = N::LAST;
  static constexpr int BODY = N::H0 * (O + 1) + N::H1 * (N::H0 + 1) + (NH == 3 ? N::H2 * (N::H1 + 1) : 0);
  static constexpr int LOG_STD = 0, PI = A, VF = PI + BODY, PI_HEAD = VF + BODY, VF_HEAD = PI_HEAD + A * (LAST + 1);
  static constexpr int P = VF_HEAD + LAST + 1;
  static constexpr int STRIDE = P + 2;  // a partial vector: the gradient, then sum(-min(s1, s2)) and sum(verr^2)
  // within a body: W0, b0, W1, b1, W2, b2
  static constexpr int W0 = 0, B0 = W0 + N::H0 * O, W1 = B0 + N::H0, B1 = W1 + N::H1 * N::H0, W2 = B1 + N::H1, B2 = W2 + N::H2 * N::H1;
};

// 16 x 16 transpose of one accumulator tile inside a wave. In: C/D layout (lane (g, e) = (lane >> 4, lane & 15), register r:
// feature 4 g + r of row e). Out: "row on the group" layout (lane (g, f), register c: feature f of row 4 c + g) -- the A
// operand (as dZ^T) and the B operand (as H) of the dW product, whose k index is the row. buf: 256 floats of this wave's own.
TB_DEV f32x4 ppo_transpose(const f32x4 c, float* buf, int lane) {
  const int g = lane >> 4, e = lane & 15;
  *reinterpret_cast<f32x4*>(buf + e * 16 + 4 * g) = c;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  f32x4 t;
#pragma unroll
  for (int k = 0; k < 4; ++k) t[k] = buf[(4 * k + g) * 16 + e];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  return t;
}

// ---------------------------------------------------------------------------------------------------------- the shared pieces
// Blocks that the tile kernels of this file and of tb_trpo.hpp used to repeat, defined once. A kernel that calls one computes the
// same float operations in the same order as every other caller.
//   piece                        called by                                        order and precision
//   PpoForward                   PpoLayer (so every tower), TrpoFwd               z = bias, then += W x chunk by chunk, c ascending: fp32 MFMA
//   ppo_row, ppo_tile            tb_trpo_fvp_kernel, tb_trpo_search_kernel        entry min(i, B - 1) of the index vector, clamped to
//                                (ppo_row alone: tb_ppo_adv_stats_kernel)         [0, n_rows); a slot past the batch repeats the last
//                                                                                 entry and is masked by `valid`
//   ppo_adv_norm                 tb_trpo_search_kernel                            the 64 float64 pairs in block order 0 .. 63; mean, variance
//                                                                                 and sqrt in float64; then (float)mean, (float)std + 1e-8f
//   ppo_backward (_head, _step,  tb_trpo_fvp_kernel                               dz = dh (1 - h^2); dh_in = W^T dz on the MFMA, (t, r)
//   _first)                                                                       ascending; dW += dz^T h_in over the tile's rows, 4 per MFMA;
//                                                                                 db as in PpoLayer::accumulate. Layers from the head down
//   ppo_partial_run / _total     tb_ppo_reduce_kernel, tb_trpo_fvp_reduce_kernel  float64: four runs of n_part / 4 partial vectors in
//                                                                                 order, then (0 + 1) + (2 + 3)
// ppo_tower and ppo_tuned_tower do NOT call ppo_tile, ppo_adv_norm or ppo_backward, nor tb_ppo_reduce_tuned_kernel the partial sum:
// they spell the same operations out themselves (see ppo_tower), and tests/test_gpu_learner_bits.py holds them and the callers above
// to one set of recorded bits.

// the clamped row of entry min(i, B - 1) of an index vector
TB_DEV long long ppo_row(const long long* idx, int i, int B, long long n_rows) {
  const long long row = idx[i < B ? i : B - 1];
  return row < 0 ? 0 : row >= n_rows ? n_rows - 1 : row;
}

// the 16 rows i0 .. i0 + 15 of a tile for this lane (g, e): slot e's row (returned; `valid`: inside the batch) and its observation
// as the first layer's k-chunks x0[c] = obs[row][4 c + g] ...
template <int O, int NC>
TB_DEV long long ppo_tile(const float* obs, const long long* idx, int i0, int B, long long n_rows, int lane, bool& valid, float (&x0)[NC]) {
  const int g = lane >> 4, e = lane & 15;
  valid = i0 + e < B;
  const long long row = ppo_row(idx, i0 + e, B, n_rows);
  const float* orow = obs + (size_t)row * O;
#pragma unroll
  for (int c = 0; c < NC; ++c) x0[c] = 4 * c + g < O ? orow[4 * c + g] : 0.0f;
  return row;
}
// ... and, for a backward pass, the observations in ppo_transpose's layout: obsT[0][c] = feature e of slot 4 c + g's row
template <int O, int NC>
TB_DEV long long ppo_tile(const float* obs, const long long* idx, int i0, int B, long long n_rows, int lane, bool& valid, float (&x0)[NC], f32x4 (&obsT)[1]) {
  const int g = lane >> 4, e = lane & 15;
  const long long row = ppo_tile<O>(obs, idx, i0, B, n_rows, lane, valid, x0);
#pragma unroll
  for (int c = 0; c < 4; ++c) obsT[0][c] = e < O ? obs[(size_t)ppo_row(idx, i0 + 4 * c + g, B, n_rows) * O + e] : 0.0f;
  return row;
}

// the minibatch's advantage mean and unbiased std + 1e-8 from tb_ppo_adv_stats_kernel's float64 sums
struct PpoAdvNorm { float mean, den; };
TB_DEV PpoAdvNorm ppo_adv_norm(const double* adv_sums, int B) {
  double sx = 0.0, sq = 0.0;
  for (int k = 0; k < TB_PPO_STAT_BLOCKS; ++k) { sx += adv_sums[2 * k]; sq += adv_sums[2 * k + 1]; }
  const double mean = sx / (double)B, var = (sq - sx * mean) / (double)(B - 1);
  return {(float)mean, (float)sqrt(var > 0.0 ? var : 0.0) + 1e-8f};
}

// The float64 sum over the n_part partial vectors of slot p by a 4 x 64 workgroup: thread (q, j) adds quarter q in order
// (ppo_partial_run) into s_sum[q][j]; after a barrier the slot's total is (0 + 1) + (2 + 3) (ppo_partial_total).
TB_DEV double ppo_partial_run(const float* partials, size_t stride, int p, int n_part, int q) {
  const int per = (n_part + 3) / 4, lo = q * per, hi = lo + per < n_part ? lo + per : n_part;
  double s = 0.0;
  for (int k = lo; k < hi; ++k) s += (double)partials[(size_t)k * stride + p];
  return s;
}
TB_DEV double ppo_partial_total(const double (&s_sum)[4][64], int j) { return (s_sum[0][j] + s_sum[1][j]) + (s_sum[2][j] + s_sum[3][j]); }

// the forward half of one nn.Linear for this lane: forward fragments and bias
template <int IN, int OUT, bool FIRST>
struct PpoForward {
  // (a later layer's input is whole accumulator tiles: IN is a multiple of 16, or -- the tuned net's feature -- narrower than one tile,
  //  the tile's other rows being exact zeros that meet zero weights)
  static constexpr int NT = (OUT + 15) / 16, NTI = (IN + 15) / 16, NC = FIRST ? (IN + 3) / 4 : NTI * 4;
  static_assert(FIRST || IN % 16 == 0 || IN < 16, "hidden widths are multiples of 16");
  float wf[NT * NC];                   // (t, c): W[16 t + j][k(c, g)], k as in tb_policy.hpp
  f32x4 bias[NT];
  // z = bias + W x. The first layer takes its k-chunks as floats, the later ones the previous layer's C/D registers
  TB_DEV void forward_first(const float (&x)[NC], f32x4 (&z)[NT]) const {
#pragma unroll
    for (int t = 0; t < NT; ++t) z[t] = bias[t];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
#pragma unroll
      for (int t = 0; t < NT; ++t) z[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[t * NC + c], x[c], z[t], 0, 0, 0);
    }
  }
  TB_DEV void forward(const f32x4 (&h)[NTI], f32x4 (&z)[NT]) const {
#pragma unroll
    for (int t = 0; t < NT; ++t) z[t] = bias[t];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
#pragma unroll
      for (int t = 0; t < NT; ++t) z[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[t * NC + c], h[c >> 2][c & 3], z[t], 0, 0, 0);
    }
  }
};

// one nn.Linear of a tower for this lane: PpoForward, the transposed fragments, and the gradient accumulators
// WB_REGS = false (the tuned net's extractor output layer and third tower layer: six layers' operands do not fit in 512 registers): the transposed fragments
// live in the wave's own LDS instead (stage_wb / backward_input_lds)
template <int IN, int OUT, bool FIRST, bool WB_REGS = true>
struct PpoLayer : PpoForward<IN, OUT, FIRST> {
  using Fwd = PpoForward<IN, OUT, FIRST>;
  using Fwd::wf;
  using Fwd::bias;
  static constexpr int NT = Fwd::NT, NTI = Fwd::NTI, NC = Fwd::NC;
  static constexpr int NWB = NTI * NT * 4;
  float wb[FIRST || !WB_REGS ? 1 : NWB];  // (ti, t, r): W[16 t + 4 g + r][16 ti + j]
  f32x4 dw[NT * NTI];                  // (t, ti), C/D layout: dW[16 t + 4 g + r][16 ti + j]
  float db[NT];                        // feature 16 t + j, summed over the rows = g (mod 4) so far

  TB_DEV void load(const float* W, const float* b, int lane) {
    const int g = lane >> 4, j = lane & 15;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int o = 16 * t + j, k = FIRST ? 4 * c + g : 16 * (c >> 2) + 4 * g + (c & 3);
        wf[t * NC + c] = (o < OUT && k < IN) ? W[o * IN + k] : 0.0f;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o = 16 * t + 4 * g + r;
        bias[t][r] = o < OUT ? b[o] : 0.0f;
      }
      db[t] = 0.0f;
#pragma unroll
      for (int ti = 0; ti < NTI; ++ti) dw[t * NTI + ti] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }
    if (!FIRST && WB_REGS) {
#pragma unroll
      for (int ti = 0; ti < NTI; ++ti) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int o = 16 * t + 4 * g + r, i = 16 * ti + j;
            wb[(ti * NT + t) * 4 + r] = (o < OUT && i < IN) ? W[o * IN + i] : 0.0f;
          }
        }
      }
    }
  }
  // the transposed fragments into lds[NWB][64] of this wave's own (written and read by the same lane: no barrier)
  TB_DEV void stage_wb(const float* W, float* lds, int lane) const {
    const int g = lane >> 4, j = lane & 15;
#pragma unroll
    for (int ti = 0; ti < NTI; ++ti) {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int o = 16 * t + 4 * g + r, i = 16 * ti + j;
          lds[((ti * NT + t) * 4 + r) * 64 + lane] = (o < OUT && i < IN) ? W[o * IN + i] : 0.0f;
        }
      }
    }
  }
  TB_DEV void backward_input_lds(const float* lds, int lane, const f32x4 (&dz)[NT], f32x4 (&dh)[NTI]) const {
#pragma unroll
    for (int ti = 0; ti < NTI; ++ti) dh[ti] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int ti = 0; ti < NTI; ++ti) dh[ti] = __builtin_amdgcn_mfma_f32_16x16x4f32(lds[((ti * NT + t) * 4 + r) * 64 + lane], dz[t][r], dh[ti], 0, 0, 0);
      }
    }
  }
  // dh = W^T dz, in the C/D layout of this layer's input
  TB_DEV void backward_input(const f32x4 (&dz)[NT], f32x4 (&dh)[NTI]) const {
#pragma unroll
    for (int ti = 0; ti < NTI; ++ti) dh[ti] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int ti = 0; ti < NTI; ++ti) dh[ti] = __builtin_amdgcn_mfma_f32_16x16x4f32(wb[(ti * NT + t) * 4 + r], dz[t][r], dh[ti], 0, 0, 0);
      }
    }
  }
  // dW += dz^T h, db += dz^T 1 for the tile's 16 rows; both operands in ppo_transpose's layout
  TB_DEV void accumulate(const f32x4 (&dzT)[NT], const f32x4 (&hT)[NTI]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int ti = 0; ti < NTI; ++ti) dw[t * NTI + ti] = __builtin_amdgcn_mfma_f32_16x16x4f32(dzT[t][c], hT[ti][c], dw[t * NTI + ti], 0, 0, 0);
      }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) db[t] += (dzT[t][0] + dzT[t][1]) + (dzT[t][2] + dzT[t][3]);
  }
  // this wave's sums into its partial vector (gW, gb: where this layer's weight and bias lie in it)
  TB_DEV void store(float* gW, float* gb, int lane) const {
    const int g = lane >> 4, j = lane & 15;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
      for (int ti = 0; ti < NTI; ++ti) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int o = 16 * t + 4 * g + r, i = 16 * ti + j;
          if (o < OUT && i < IN) gW[o * IN + i] = dw[t * NTI + ti][r];
        }
      }
      float s = db[t];  // the four lane groups hold the rows = 0, 1, 2, 3 (mod 4): (0 + 1) + (2 + 3) on every lane
      s += __shfl_xor(s, 16);
      s += __shfl_xor(s, 32);
      if (g == 0 && 16 * t + j < OUT) gb[16 * t + j] = s;
    }
  }
};

template <int NTILES>
TB_DEV void ppo_tanh(const f32x4 (&z)[NTILES], f32x4 (&h)[NTILES]) {
#pragma unroll
  for (int t = 0; t < NTILES; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) h[t][r] = fast_tanh(z[t][r]);
  }
}
// dz = dh (1 - h^2)
template <int NTILES>
TB_DEV void ppo_dtanh(const f32x4 (&dh)[NTILES], const f32x4 (&h)[NTILES], f32x4 (&dz)[NTILES]) {
#pragma unroll
  for (int t = 0; t < NTILES; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) dz[t][r] = dh[t][r] * (1.0f - h[t][r] * h[t][r]);
  }
}
template <int NTILES>
TB_DEV void ppo_transpose_all(const f32x4 (&c)[NTILES], f32x4 (&t)[NTILES], float* buf, int lane) {
#pragma unroll
  for (int k = 0; k < NTILES; ++k) t[k] = ppo_transpose(c[k], buf + (k & 1) * 256, lane);
}

// The backward pass of one tile of a tanh tower, layer by layer from the head down. l: a PpoLayer; dz: the loss's derivative with
// respect to its output; h_in / dh_in: its input and the derivative with respect to it (C/D layout); buf: ppo_transpose's 512 floats.
// the head (no activation behind it; dz = dout): dh_in = W^T dz; dW += dz^T h_in; db += dz^T 1
template <class LAYER>
TB_DEV void ppo_backward_head(LAYER& l, const f32x4 (&dz)[1], const f32x4 (&h_in)[LAYER::NTI], f32x4 (&dh_in)[LAYER::NTI], float* buf, int lane) {
  f32x4 dzT[1], hT[LAYER::NTI];
  ppo_transpose_all(dz, dzT, buf, lane);
  l.backward_input(dz, dh_in);
  ppo_transpose_all(h_in, hT, buf, lane);
  l.accumulate(dzT, hT);
}
// a hidden layer with output h = tanh(z): dz = dh (1 - h^2), then the same three
template <class LAYER>
TB_DEV void ppo_backward_step(LAYER& l, const f32x4 (&dh)[LAYER::NT], const f32x4 (&h)[LAYER::NT], const f32x4 (&h_in)[LAYER::NTI], f32x4 (&dh_in)[LAYER::NTI],
                              float* buf, int lane) {
  f32x4 dz[LAYER::NT], dzT[LAYER::NT], hT[LAYER::NTI];
  ppo_dtanh(dh, h, dz);
  l.backward_input(dz, dh_in);
  ppo_transpose_all(dz, dzT, buf, lane); ppo_transpose_all(h_in, hT, buf, lane);
  l.accumulate(dzT, hT);
}
// the first layer: nothing to send further back, and its input arrives transposed (ppo_tile's obsT)
template <class LAYER>
TB_DEV void ppo_backward_first(LAYER& l, const f32x4 (&dh)[LAYER::NT], const f32x4 (&h)[LAYER::NT], const f32x4 (&obsT)[1], float* buf, int lane) {
  f32x4 dz[LAYER::NT], dzT[LAYER::NT];
  ppo_dtanh(dh, h, dz);
  ppo_transpose_all(dz, dzT, buf, lane);
  l.accumulate(dzT, obsT);
}
// NH hidden layers (l2 and h2 are untouched when NH == 2): head, hidden layers, first layer
template <int NH, class L0, class L1, class L2, class LH>
TB_DEV void ppo_backward(L0& l0, L1& l1, L2& l2, LH& lh, const f32x4 (&dout)[1], const f32x4 (&obsT)[1], const f32x4 (&h0)[L0::NT], const f32x4 (&h1)[L1::NT],
                         const f32x4 (&h2)[L2::NT], float* buf, int lane) {
  f32x4 dh1[L1::NT], dh0[L0::NT];
  if constexpr (NH == 3) {
    f32x4 dh2[L2::NT];
    ppo_backward_head(lh, dout, h2, dh2, buf, lane);
    ppo_backward_step(l2, dh2, h2, h1, dh1, buf, lane);
  } else {
    ppo_backward_head(lh, dout, h1, dh1, buf, lane);
  }
  ppo_backward_step(l1, dh1, h1, h0, dh0, buf, lane);
  ppo_backward_first(l0, dh0, h0, obsT, buf, lane);
}

struct PpoGradArgs {
  const float* obs;       // [N][O]
  const float* act;       // [N][A] the unclipped samples
  const float* old_logp;  // [N]
  const float* adv;       // [N]
  const float* ret;       // [N]
  const long long* idx;   // [B] rows of the minibatch
  const float* params;    // [P]
  const double* adv_sums; // [TB_PPO_STAT_BLOCKS][2]: sum x, sum x^2 of adv[idx]
  float* partials;        // [2 * workgroups][P + 2]
  long long n_rows;
  int batch;
  float clip_range, vf_coef;
};

// ---- THE MEMBER AXIS (tb_ppo_grad_members / tb_ppo_apply_members: a population of PPO learners takes its minibatch step in three
// launches, whatever its size). The flat rollout arrays are shared; a member's rows are picked by ITS index row. Per member: an
// index row, a parameter / gradient / moment row, a workspace region (advantage sums, then partials), a statistics row [3] and a
// hyper-parameter row (TbPpoMemberHp: clip_range, vf_coef, ent_coef, lr). Every kernel below takes the member as ONE trailing
// argument, a PpoMembers, in a pack that is empty or holds that one: with the pack empty the kernel is what it was, argument list
// included. With it, the member is blockIdx.y (blockIdx.x of the one-workgroup step kernel); a prologue offsets the member's own
// pointers and takes its scalars from hp[member]; the body -- every reduction order, the absence of atomics, the arithmetic -- is the
// same lines. The member index depends on the block index alone: every offset pointer stays scalar.
struct PpoMembers {
  const TbPpoMemberHp* hp;  // [M]
  size_t idx_stride;        // int64 entries between index rows
  size_t param_stride;      // floats between parameter (gradient, moment) rows
  size_t ws_stride;         // bytes between workspace regions (a multiple of 8)
};
template <class T> TB_DEV T* ppo_member_bytes(T* p, size_t bytes) { return (T*)((const char*)p + bytes); }

// sum and sum of squares of the minibatch's advantages, float64, one pair per block (fixed order inside a block)
template <class... MEMBERS>
__global__ __launch_bounds__(256) void tb_ppo_adv_stats_kernel(const float* adv, const long long* idx, int batch, long long n_rows, double* out, MEMBERS... members) {
  static_assert(sizeof...(MEMBERS) <= 1, "no argument, or one PpoMembers");
  if constexpr (sizeof...(MEMBERS) != 0) {
    const PpoMembers mb = (members, ...);
    idx += (size_t)blockIdx.y * mb.idx_stride;
    out = ppo_member_bytes(out, (size_t)blockIdx.y * mb.ws_stride);
  }
  __shared__ double s_x[256], s_q[256];
  double x = 0.0, q = 0.0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < batch; i += TB_PPO_STAT_BLOCKS * 256) {
    const double a = (double)adv[ppo_row(idx, i, batch, n_rows)];
    x += a; q += a * a;
  }
  s_x[threadIdx.x] = x; s_q[threadIdx.x] = q;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) { s_x[threadIdx.x] += s_x[threadIdx.x + w]; s_q[threadIdx.x] += s_q[threadIdx.x + w]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { out[2 * blockIdx.x] = s_x[0]; out[2 * blockIdx.x + 1] = s_q[0]; }
}

// one tower of one half share. PI: the policy tower (logp, ratio, clipped surrogate, d log_std); else the value tower.
// This tower and ppo_tuned_tower keep their own text of the clamp, the tile gather, the advantage norm and the backward chain: the
// max-ILP scheduler orders these two 500-register waves differently for any change of their source. With ppo_tile, a shared loss
// head and ppo_backward tb_ppo_grad_kernel<SWING> ran 2.6 % slower, with ppo_row alone both towers' streams already differ; as they
// stand all eight gradient kernels compile to the parent's instruction stream ("Shared learner pieces").
template <int KIND, bool PI, int NET = TB_NET_DEFAULT>
TB_DEV void ppo_tower(const PpoGradArgs& a, float* buf, int lane, int first, float* part) {
  using L = PpoLayout<KIND, NET>;
  using N = PolicyNet<KIND, NET>;
  constexpr int O = L::O, NA = L::A, NH = L::NH, HOUT = PI ? NA : 1;
  const int g = lane >> 4, e = lane & 15, B = a.batch;
  const float* body = a.params + (PI ? L::PI : L::VF);
  const float* head = a.params + (PI ? L::PI_HEAD : L::VF_HEAD);
  using L0 = PpoLayer<O, N::H0, true>;
  using L1 = PpoLayer<N::H0, N::H1, false>;
  using L2 = PpoLayer<N::H1, N::H2, false>;  // (untouched when NH == 2)
  using LH = PpoLayer<N::LAST, HOUT, false>;
  L0 l0;
  L1 l1;
  L2 l2;
  LH lh;
  l0.load(body + L::W0, body + L::B0, lane);
  l1.load(body + L::W1, body + L::B1, lane);
  if (NH == 3) l2.load(body + L::W2, body + L::B2, lane);
  lh.load(head, head + HOUT * N::LAST, lane);

  // the minibatch's advantage mean and unbiased std (PI), from the pre-pass' float64 sums in a fixed order
  float adv_mean = 0.0f, adv_den = 1.0f;
  float ls[4], inv_std[4], dls[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (PI) {
    double sx = 0.0, sq = 0.0;
    for (int k = 0; k < TB_PPO_STAT_BLOCKS; ++k) { sx += a.adv_sums[2 * k]; sq += a.adv_sums[2 * k + 1]; }
    const double mean = sx / (double)B, var = (sq - sx * mean) / (double)(B - 1);
    adv_mean = (float)mean;
    adv_den = (float)sqrt(var > 0.0 ? var : 0.0) + 1e-8f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      ls[r] = 4 * g + r < NA ? a.params[L::LOG_STD + 4 * g + r] : 0.0f;
      inv_std[r] = expf(-ls[r]);
    }
  }
  const float fb = (float)B;
  float stat = 0.0f;  // PI: sum of -min(s1, s2); else sum of verr^2 (this lane's rows; lanes of group 0 only)

  for (int i0 = first; i0 < first + TB_PPO_HALF && i0 < B; i0 += 16) {
    // rows of the tile: slot e for the C/D layout, slots 4 c + g for the transposed one
    const bool valid = i0 + e < B;
    long long row = a.idx[valid ? i0 + e : B - 1];
    row = row < 0 ? 0 : row >= a.n_rows ? a.n_rows - 1 : row;
    float x0[L0::NC];
    const float* orow = a.obs + (size_t)row * O;
#pragma unroll
    for (int c = 0; c < L0::NC; ++c) x0[c] = 4 * c + g < O ? orow[4 * c + g] : 0.0f;
    f32x4 obsT[1];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int s = i0 + 4 * c + g;
      long long rc = a.idx[s < B ? s : B - 1];
      rc = rc < 0 ? 0 : rc >= a.n_rows ? a.n_rows - 1 : rc;
      obsT[0][c] = e < O ? a.obs[(size_t)rc * O + e] : 0.0f;
    }
    // forward
    f32x4 z0[L0::NT], h0[L0::NT], z1[L1::NT], h1[L1::NT], z2[L2::NT], h2[L2::NT], zh[1];
    l0.forward_first(x0, z0); ppo_tanh(z0, h0);
    l1.forward(h0, z1); ppo_tanh(z1, h1);
    if constexpr (NH == 3) {
      l2.forward(h1, z2); ppo_tanh(z2, h2);
      lh.forward(h2, zh);
    } else {
      lh.forward(h1, zh);
    }
    // the loss's derivative with respect to the head's output (C/D layout: register r = output 4 g + r of row e)
    f32x4 dout[1] = {f32x4{0.0f, 0.0f, 0.0f, 0.0f}};
    if constexpr (PI) {
      float zeta[4], lp = 0.0f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool on = 4 * g + r < NA;
        const float raw = on ? a.act[(size_t)row * NA + 4 * g + r] : 0.0f;
        zeta[r] = on ? (raw - zh[0][r]) * inv_std[r] : 0.0f;
        if (on) lp += (-0.5f * zeta[r] * zeta[r] - ls[r]) - TB_LN_SQRT_2PI;
      }
      lp += __shfl_xor(lp, 16);
      lp += __shfl_xor(lp, 32);
      const float ratio = expf(lp - a.old_logp[row]);
      const float an = (a.adv[row] - adv_mean) / adv_den;
      const float s1 = an * ratio, s2 = an * fminf(fmaxf(ratio, 1.0f - a.clip_range), 1.0f + a.clip_range);
      const bool active = s1 <= s2;
      if (valid && g == 0) stat += -fminf(s1, s2);
      const float d_logp = (valid && active) ? (-an * ratio) / fb : 0.0f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        dout[0][r] = (d_logp * zeta[r]) * inv_std[r];
        dls[r] += d_logp * (zeta[r] * zeta[r] - 1.0f);
      }
    } else {
      const float verr = valid ? a.ret[row] - zh[0][0] : 0.0f;
      if (g == 0) {
        stat += verr * verr;
        dout[0][0] = (-2.0f * a.vf_coef / fb) * verr;
      }
    }
    // backward
    f32x4 doutT[1];
    ppo_transpose_all(dout, doutT, buf, lane);
    if constexpr (NH == 3) {
      f32x4 dh2[L2::NT], dz2[L2::NT], dz2T[L2::NT], h2T[L2::NT], dh1[L1::NT], dz1[L1::NT], dz1T[L1::NT], h1T[L1::NT], dh0[L0::NT], dz0[L0::NT], dz0T[L0::NT], h0T[L0::NT];
      lh.backward_input(dout, dh2);
      ppo_transpose_all(h2, h2T, buf, lane);
      lh.accumulate(doutT, h2T);
      ppo_dtanh(dh2, h2, dz2);
      l2.backward_input(dz2, dh1);
      ppo_transpose_all(dz2, dz2T, buf, lane); ppo_transpose_all(h1, h1T, buf, lane);
      l2.accumulate(dz2T, h1T);
      ppo_dtanh(dh1, h1, dz1);
      l1.backward_input(dz1, dh0);
      ppo_transpose_all(dz1, dz1T, buf, lane); ppo_transpose_all(h0, h0T, buf, lane);
      l1.accumulate(dz1T, h0T);
      ppo_dtanh(dh0, h0, dz0);
      ppo_transpose_all(dz0, dz0T, buf, lane);
      l0.accumulate(dz0T, obsT);
    } else {
      f32x4 dh1[L1::NT], dz1[L1::NT], dz1T[L1::NT], h1T[L1::NT], dh0[L0::NT], dz0[L0::NT], dz0T[L0::NT], h0T[L0::NT];
      lh.backward_input(dout, dh1);
      ppo_transpose_all(h1, h1T, buf, lane);
      lh.accumulate(doutT, h1T);
      ppo_dtanh(dh1, h1, dz1);
      l1.backward_input(dz1, dh0);
      ppo_transpose_all(dz1, dz1T, buf, lane); ppo_transpose_all(h0, h0T, buf, lane);
      l1.accumulate(dz1T, h0T);
      ppo_dtanh(dh0, h0, dz0);
      ppo_transpose_all(dz0, dz0T, buf, lane);
      l0.accumulate(dz0T, obsT);
    }
  }

  // this wave's slots of the partial vector
  float* gbody = part + (PI ? L::PI : L::VF);
  float* ghead = part + (PI ? L::PI_HEAD : L::VF_HEAD);
  l0.store(gbody + L::W0, gbody + L::B0, lane);
  l1.store(gbody + L::W1, gbody + L::B1, lane);
  if (NH == 3) l2.store(gbody + L::W2, gbody + L::B2, lane);
  lh.store(ghead, ghead + HOUT * N::LAST, lane);
#pragma unroll
  for (int w = 1; w < 16; w <<= 1) {  // over the 16 rows of a lane group
    stat += __shfl_xor(stat, w);
    if (PI) {
#pragma unroll
      for (int r = 0; r < 4; ++r) dls[r] += __shfl_xor(dls[r], w);
    }
  }
  if (PI && e == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (4 * g + r < NA) part[L::LOG_STD + 4 * g + r] = dls[r];
    }
  }
  if (lane == 0) part[L::P + (PI ? 0 : 1)] = stat;
}

// the member's view of the shared arguments: its index row, parameter row, workspace region (sums, then partials), clip_range, vf_coef
TB_DEV void ppo_member_args(PpoGradArgs& a, const PpoMembers& mb) {
  const size_t m = blockIdx.y;
  a.idx += m * mb.idx_stride;
  a.params += m * mb.param_stride;
  a.adv_sums = ppo_member_bytes(a.adv_sums, m * mb.ws_stride);
  a.partials = ppo_member_bytes(a.partials, m * mb.ws_stride);
  a.clip_range = mb.hp[m].clip_range;
  a.vf_coef = mb.hp[m].vf_coef;
}

template <int KIND, int NET = TB_NET_DEFAULT, class... MEMBERS>
__global__ __launch_bounds__(256) void tb_ppo_grad_kernel(PpoGradArgs a, MEMBERS... members) {
  static_assert(sizeof...(MEMBERS) <= 1, "no argument, or one PpoMembers");
  if constexpr (sizeof...(MEMBERS) != 0) ppo_member_args(a, members...);
  __shared__ __attribute__((aligned(16))) float s_buf[4 * 512];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = wave & 1;
  const int first = blockIdx.x * TB_PPO_SHARE + half * TB_PPO_HALF;
  float* part = a.partials + (size_t)(2 * blockIdx.x + half) * PpoLayout<KIND, NET>::STRIDE;
  if (wave < 2) ppo_tower<KIND, true, NET>(a, s_buf + wave * 512, lane, first, part);
  else ppo_tower<KIND, false, NET>(a, s_buf + wave * 512, lane, first, part);
}

// gradient[p] = sum of the partials in a fixed order (ppo_partial_run / ppo_partial_total); log_std's
// entropy term; the minibatch's three statistics. 64 parameters per block. value_only: grad's policy slots (log_std, PI,
// PI_HEAD) are left as they are.
// the member's partials, parameter and gradient rows, statistics row, ent_coef
TB_DEV void ppo_member_reduce(const PpoMembers& mb, const float*& partials, const float*& params, float& ent_coef, float*& grad, float*& stats) {
  const size_t m = blockIdx.y;
  partials = ppo_member_bytes(partials, m * mb.ws_stride);
  params += m * mb.param_stride;
  grad += m * mb.param_stride;
  stats += 3 * m;
  ent_coef = mb.hp[m].ent_coef;
}

template <int KIND, int NET = TB_NET_DEFAULT, class... MEMBERS>
__global__ __launch_bounds__(256) void tb_ppo_reduce_kernel(const float* partials, int n_part, int batch, const float* params, float ent_coef, float* grad,
                                                            float* stats, int value_only, MEMBERS... members) {
  static_assert(sizeof...(MEMBERS) <= 1, "no argument, or one PpoMembers");
  if constexpr (sizeof...(MEMBERS) != 0) ppo_member_reduce((members, ...), partials, params, ent_coef, grad, stats);
  using L = PpoLayout<KIND, NET>;
  __shared__ double s_sum[4][64];
  const int j = threadIdx.x & 63, q = threadIdx.x >> 6, p = blockIdx.x * 64 + j;
  s_sum[q][j] = p < L::STRIDE ? ppo_partial_run(partials, L::STRIDE, p, n_part, q) : 0.0;
  __syncthreads();
  if (q == 0 && p < L::STRIDE) {
    const double total = ppo_partial_total(s_sum, j);
    if (p < L::P) {
      const bool value_slot = (p >= L::VF && p < L::PI_HEAD) || p >= L::VF_HEAD;
      if (!value_only || value_slot) grad[p] = p < L::A ? (float)total - ent_coef : (float)total;
    } else {
      stats[p - L::P] = (float)(total / (double)batch);
      if (p == L::P) {
        float ent = 0.0f;
        for (int k = 0; k < L::A; ++k) ent += (0.5f + TB_LN_SQRT_2PI) + params[L::LOG_STD + k];
        stats[2] = ent;
      }
    }
  }
}

// grad /= world; the global norm (float64, fixed-order tree); torch's clip factor; Adam. One workgroup. Only the slots in
// [lo0, hi0) or [lo1, hi1) take part, in the norm too (every slot: 0, P, 0, 0; the critic alone: the VF and VF_HEAD slots).
// The members form: one workgroup per member (blockIdx.x), its four rows and its lr.
template <class... MEMBERS>
__global__ __launch_bounds__(1024) void tb_ppo_step_kernel(float* params, float* grad, float* m, float* v, int P, float world, float max_norm, float lr,
                                                           float beta1, float beta2, float eps, float c1, float c2, int lo0, int hi0, int lo1, int hi1,
                                                           MEMBERS... members) {
  static_assert(sizeof...(MEMBERS) <= 1, "no argument, or one PpoMembers");
  if constexpr (sizeof...(MEMBERS) != 0) {
    const PpoMembers mb = (members, ...);
    const size_t row = (size_t)blockIdx.x * mb.param_stride;
    params += row; grad += row; m += row; v += row;
    lr = mb.hp[blockIdx.x].lr;
  }
  __shared__ double s_sq[1024];
  double sq = 0.0;
  for (int p = threadIdx.x; p < P; p += 1024) {
    if (!((p >= lo0 && p < hi0) || (p >= lo1 && p < hi1))) continue;
    const float g = world != 1.0f ? grad[p] / world : grad[p];
    sq += (double)g * (double)g;
  }
  s_sq[threadIdx.x] = sq;
  __syncthreads();
  for (int w = 512; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) s_sq[threadIdx.x] += s_sq[threadIdx.x + w];
    __syncthreads();
  }
  const float norm = (float)sqrt(s_sq[0]);
  const float r = max_norm / (norm + 1e-6f);
  const float coef = r < 1.0f ? r : (r != r ? r : 1.0f);  // torch's clamp(max = 1): a NaN stays (fminf would drop it)
  for (int p = threadIdx.x; p < P; p += 1024) {
    if (!((p >= lo0 && p < hi0) || (p >= lo1 && p < hi1))) continue;
    const float g = (world != 1.0f ? grad[p] / world : grad[p]) * coef;
    const float mk = beta1 * m[p] + (1.0f - beta1) * g;
    const float vk = beta2 * v[p] + ((1.0f - beta2) * g) * g;
    grad[p] = g; m[p] = mk; v[p] = vk;
    params[p] = params[p] - lr * (mk / c1) / (sqrtf(vk / c2) + eps);
  }
}

// GAE: one lane per env, backwards over the steps; a step's loads and stores coalesce across envs. Operation for operation
// PPOTrainer.advantages: delta = r + (gamma V') nt - V, g = delta + (c nt) g with c = fl(gamma lambda), returns = g + V.
__global__ __launch_bounds__(64) void tb_ppo_gae_kernel(int T, int n, const float* rew, size_t rew_stride, const unsigned char* done, size_t done_stride,
                                                        const float* values, const float* last_value, float gamma, float c, float* adv, float* ret) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  float next = last_value[i], g = 0.0f;
#pragma unroll 8
  for (int k = T - 1; k >= 0; --k) {
    const float nt = done[(size_t)k * done_stride + i] ? 0.0f : 1.0f;
    const float V = values[(size_t)k * n + i];
    const float delta = (rew[(size_t)k * rew_stride + i] + (gamma * next) * nt) - V;
    g = delta + (c * nt) * g;
    adv[(size_t)k * n + i] = g;
    ret[(size_t)k * n + i] = g + V;
    next = V;
  }
}

// ------------------------------------------------------------------------------------------------------------------ the tuned net
// TB_NET_TUNED (Tennisbot; TunedNet in tb_policy.hpp): flat order log_std | extractor W0 b0 W1 b1 | policy_net | value_net_body |
// action_net | value_net. The two tower waves of a half share both run the shared extractor forward and send their tower's
// gradient back through it, so BOTH hold an extractor gradient: the pi wave writes its share to the extractor's own slots of the
// partial vector, the vf wave to a second extractor region behind the two statistics (EXT2), and tb_ppo_reduce_tuned_kernel adds
// the two regions' float64 sums, pi's first. No atomics, no workgroup barrier, one fixed order.
struct TunedLayout {
  using N = TunedNet;
  static constexpr int O = N::O, A = N::F;
  static constexpr int EXT_SIZE = N::FH * (O + 1) + A * (N::FH + 1);
  static constexpr int BODY = N::H0 * (A + 1) + N::H1 * (N::H0 + 1) + N::H2 * (N::H1 + 1);
  static constexpr int LOG_STD = 0, EXT = A, PI = EXT + EXT_SIZE, VF = PI + BODY, PI_HEAD = VF + BODY, VF_HEAD = PI_HEAD + A * (N::H2 + 1);
  static constexpr int P = VF_HEAD + N::H2 + 1;
  static constexpr int EXT2 = P + 2, STRIDE = EXT2 + EXT_SIZE;  // gradient, the two statistics, the vf wave's extractor share
  // within the extractor: W0, b0, W1, b1; within a body: W0, b0, W1, b1, W2, b2
  static constexpr int EW0 = 0, EB0 = EW0 + N::FH * O, EW1 = EB0 + N::FH, EB1 = EW1 + A * N::FH;
  static constexpr int W0 = 0, B0 = W0 + N::H0 * A, W1 = B0 + N::H0, B1 = W1 + N::H1 * N::H0, W2 = B1 + N::H1, B2 = W2 + N::H2 * N::H1;
};

template <int NTILES>
TB_DEV void ppo_relu(const f32x4 (&z)[NTILES], f32x4 (&h)[NTILES]) {
#pragma unroll
  for (int t = 0; t < NTILES; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) h[t][r] = relu(z[t][r]);
  }
}
// dz = dh where the unit is on (h > 0 exactly where z > 0), 0 where z <= 0
template <int NTILES>
TB_DEV void ppo_drelu(const f32x4 (&dh)[NTILES], const f32x4 (&h)[NTILES], f32x4 (&dz)[NTILES]) {
#pragma unroll
  for (int t = 0; t < NTILES; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) dz[t][r] = h[t][r] > 0.0f ? dh[t][r] : 0.0f;
  }
}

// one tower of one half share, extractor included: forward through extractor and tower, backward through both.
// TB_TUNED_STAGE: a scheduling fence between the stages of a tile. Left alone the max-ILP scheduler interleaves a layer's backward
// products with the next layer's transposes and keeps both layers' temporaries alive: 2-7 VGPRs spilled at the 512-register limit.
#define TB_TUNED_STAGE() __builtin_amdgcn_sched_barrier(0)
template <bool PI>
TB_DEV void ppo_tuned_tower(const PpoGradArgs& a, float* buf, float* wb_lds, int lane, int first, float* part) {
  using L = TunedLayout;
  using N = TunedNet;
  constexpr int O = L::O, NA = L::A, HOUT = PI ? NA : 1;
  const int g = lane >> 4, e = lane & 15, B = a.batch;
  const float* ext = a.params + L::EXT;
  const float* body = a.params + (PI ? L::PI : L::VF);
  const float* head = a.params + (PI ? L::PI_HEAD : L::VF_HEAD);
  using E0 = PpoLayer<O, N::FH, true>;
  using E1 = PpoLayer<N::FH, N::F, false, false>;
  using L0 = PpoLayer<N::F, N::H0, false>;
  using L1 = PpoLayer<N::H0, N::H1, false>;
  using L2 = PpoLayer<N::H1, N::H2, false, false>;
  using LH = PpoLayer<N::H2, HOUT, false>;
  float* const wb2_lds = wb_lds + E1::NWB * 64;
  E0 e0;
  E1 e1;
  L0 l0;
  L1 l1;
  L2 l2;
  LH lh;
  e0.load(ext + L::EW0, ext + L::EB0, lane);
  e1.load(ext + L::EW1, ext + L::EB1, lane);
  e1.stage_wb(ext + L::EW1, wb_lds, lane);
  l0.load(body + L::W0, body + L::B0, lane);
  l1.load(body + L::W1, body + L::B1, lane);
  l2.load(body + L::W2, body + L::B2, lane);
  l2.stage_wb(body + L::W2, wb2_lds, lane);
  lh.load(head, head + HOUT * N::H2, lane);

  float adv_mean = 0.0f, adv_den = 1.0f;
  float ls[4], inv_std[4], dls[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (PI) {
    double sx = 0.0, sq = 0.0;
    for (int k = 0; k < TB_PPO_STAT_BLOCKS; ++k) { sx += a.adv_sums[2 * k]; sq += a.adv_sums[2 * k + 1]; }
    const double mean = sx / (double)B, var = (sq - sx * mean) / (double)(B - 1);
    adv_mean = (float)mean;
    adv_den = (float)sqrt(var > 0.0 ? var : 0.0) + 1e-8f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      ls[r] = 4 * g + r < NA ? a.params[L::LOG_STD + 4 * g + r] : 0.0f;
      inv_std[r] = expf(-ls[r]);
    }
  }
  const float fb = (float)B;
  float stat = 0.0f;

  for (int i0 = first; i0 < first + TB_PPO_HALF && i0 < B; i0 += 16) {
    const bool valid = i0 + e < B;
    long long row = a.idx[valid ? i0 + e : B - 1];
    row = row < 0 ? 0 : row >= a.n_rows ? a.n_rows - 1 : row;
    float x0[E0::NC];
    const float* orow = a.obs + (size_t)row * O;
#pragma unroll
    for (int c = 0; c < E0::NC; ++c) x0[c] = 4 * c + g < O ? orow[4 * c + g] : 0.0f;
    f32x4 obsT[1];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int s = i0 + 4 * c + g;
      long long rc = a.idx[s < B ? s : B - 1];
      rc = rc < 0 ? 0 : rc >= a.n_rows ? a.n_rows - 1 : rc;
      obsT[0][c] = e < O ? a.obs[(size_t)rc * O + e] : 0.0f;
    }
    // forward
    f32x4 ze[E0::NT], he[E0::NT], zf[1], f[1], z0[L0::NT], h0[L0::NT], z1[L1::NT], h1[L1::NT], z2[L2::NT], h2[L2::NT], zh[1];
    e0.forward_first(x0, ze); ppo_relu(ze, he);
    e1.forward(he, zf); ppo_relu(zf, f);
    l0.forward(f, z0); ppo_relu(z0, h0);
    l1.forward(h0, z1); ppo_relu(z1, h1);
    l2.forward(h1, z2); ppo_relu(z2, h2);
    lh.forward(h2, zh);
    TB_TUNED_STAGE();
    // the loss's derivative with respect to the head's output: ppo_tower's, term for term
    f32x4 dout[1] = {f32x4{0.0f, 0.0f, 0.0f, 0.0f}};
    if constexpr (PI) {
      float zeta[4], lp = 0.0f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool on = 4 * g + r < NA;
        const float raw = on ? a.act[(size_t)row * NA + 4 * g + r] : 0.0f;
        zeta[r] = on ? (raw - zh[0][r]) * inv_std[r] : 0.0f;
        if (on) lp += (-0.5f * zeta[r] * zeta[r] - ls[r]) - TB_LN_SQRT_2PI;
      }
      lp += __shfl_xor(lp, 16);
      lp += __shfl_xor(lp, 32);
      const float ratio = expf(lp - a.old_logp[row]);
      const float an = (a.adv[row] - adv_mean) / adv_den;
      const float s1 = an * ratio, s2 = an * fminf(fmaxf(ratio, 1.0f - a.clip_range), 1.0f + a.clip_range);
      const bool active = s1 <= s2;
      if (valid && g == 0) stat += -fminf(s1, s2);
      const float d_logp = (valid && active) ? (-an * ratio) / fb : 0.0f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        dout[0][r] = (d_logp * zeta[r]) * inv_std[r];
        dls[r] += d_logp * (zeta[r] * zeta[r] - 1.0f);
      }
    } else {
      const float verr = valid ? a.ret[row] - zh[0][0] : 0.0f;
      if (g == 0) {
        stat += verr * verr;
        dout[0][0] = (-2.0f * a.vf_coef / fb) * verr;
      }
    }
    // backward: the tower, then the extractor
    f32x4 doutT[1], dh2[L2::NT], dz2[L2::NT], dz2T[L2::NT], h2T[L2::NT], dh1[L1::NT], dz1[L1::NT], dz1T[L1::NT], h1T[L1::NT];
    f32x4 dh0[L0::NT], dz0[L0::NT], dz0T[L0::NT], h0T[L0::NT], df[1], dzf[1], dzfT[1], fT[1], dhe[E0::NT], dze[E0::NT], dzeT[E0::NT], heT[E0::NT];
    ppo_transpose_all(dout, doutT, buf, lane);
    lh.backward_input(dout, dh2);
    ppo_transpose_all(h2, h2T, buf, lane);
    lh.accumulate(doutT, h2T);
    TB_TUNED_STAGE();
    ppo_drelu(dh2, h2, dz2);
    l2.backward_input_lds(wb2_lds, lane, dz2, dh1);
    ppo_transpose_all(dz2, dz2T, buf, lane); ppo_transpose_all(h1, h1T, buf, lane);
    l2.accumulate(dz2T, h1T);
    TB_TUNED_STAGE();
    ppo_drelu(dh1, h1, dz1);
    l1.backward_input(dz1, dh0);
    ppo_transpose_all(dz1, dz1T, buf, lane); ppo_transpose_all(h0, h0T, buf, lane);
    l1.accumulate(dz1T, h0T);
    TB_TUNED_STAGE();
    ppo_drelu(dh0, h0, dz0);
    l0.backward_input(dz0, df);
    ppo_transpose_all(dz0, dz0T, buf, lane); ppo_transpose_all(f, fT, buf, lane);
    l0.accumulate(dz0T, fT);
    TB_TUNED_STAGE();
    ppo_drelu(df, f, dzf);
    e1.backward_input_lds(wb_lds, lane, dzf, dhe);
    ppo_transpose_all(dzf, dzfT, buf, lane); ppo_transpose_all(he, heT, buf, lane);
    e1.accumulate(dzfT, heT);
    TB_TUNED_STAGE();
    ppo_drelu(dhe, he, dze);
    ppo_transpose_all(dze, dzeT, buf, lane);
    e0.accumulate(dzeT, obsT);
  }

  float* gext = part + (PI ? L::EXT : L::EXT2);  // this wave's extractor share
  float* gbody = part + (PI ? L::PI : L::VF);
  float* ghead = part + (PI ? L::PI_HEAD : L::VF_HEAD);
  e0.store(gext + L::EW0, gext + L::EB0, lane);
  e1.store(gext + L::EW1, gext + L::EB1, lane);
  l0.store(gbody + L::W0, gbody + L::B0, lane);
  l1.store(gbody + L::W1, gbody + L::B1, lane);
  l2.store(gbody + L::W2, gbody + L::B2, lane);
  lh.store(ghead, ghead + HOUT * N::H2, lane);
#pragma unroll
  for (int w = 1; w < 16; w <<= 1) {
    stat += __shfl_xor(stat, w);
    if (PI) {
#pragma unroll
      for (int r = 0; r < 4; ++r) dls[r] += __shfl_xor(dls[r], w);
    }
  }
  if (PI && e == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (4 * g + r < NA) part[L::LOG_STD + 4 * g + r] = dls[r];
    }
  }
  if (lane == 0) part[L::P + (PI ? 0 : 1)] = stat;
}

#undef TB_TUNED_STAGE

template <class... MEMBERS>
__global__ __launch_bounds__(256) void tb_ppo_grad_tuned_kernel(PpoGradArgs a, MEMBERS... members) {
  static_assert(sizeof...(MEMBERS) <= 1, "no argument, or one PpoMembers");
  if constexpr (sizeof...(MEMBERS) != 0) ppo_member_args(a, members...);
  constexpr int NWB = PpoLayer<TunedNet::FH, TunedNet::F, false, false>::NWB + PpoLayer<TunedNet::H1, TunedNet::H2, false, false>::NWB;
  __shared__ __attribute__((aligned(16))) float s_buf[4 * 512];
  __shared__ float s_wb[4 * NWB * 64];  // per wave: the transposed fragments of the extractor's output layer and of the tower's third layer
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = wave & 1;
  const int first = blockIdx.x * TB_PPO_SHARE + half * TB_PPO_HALF;
  float* part = a.partials + (size_t)(2 * blockIdx.x + half) * TunedLayout::STRIDE;
  if (wave < 2) ppo_tuned_tower<true>(a, s_buf + wave * 512, s_wb + wave * NWB * 64, lane, first, part);
  else ppo_tuned_tower<false>(a, s_buf + wave * 512, s_wb + wave * NWB * 64, lane, first, part);
}

// tb_ppo_reduce_kernel for the tuned net: the same fixed-order float64 sums per slot; an extractor slot is (the sum of the pi
// waves' shares) + (the sum of the vf waves' shares, from the partials' second extractor region). Both runs of a thread sit under
// one test and one barrier; written with ppo_partial_run / ppo_partial_total the kernel compiles to another stream, so it keeps
// its own lines (the operations are those two functions')
template <class... MEMBERS>
__global__ __launch_bounds__(256) void tb_ppo_reduce_tuned_kernel(const float* partials, int n_part, int batch, const float* params, float ent_coef, float* grad,
                                                                  float* stats, MEMBERS... members) {
  static_assert(sizeof...(MEMBERS) <= 1, "no argument, or one PpoMembers");
  if constexpr (sizeof...(MEMBERS) != 0) ppo_member_reduce((members, ...), partials, params, ent_coef, grad, stats);
  using L = TunedLayout;
  __shared__ double s_sum[4][64], s_sum2[4][64];
  const int j = threadIdx.x & 63, q = threadIdx.x >> 6, p = blockIdx.x * 64 + j;
  const bool shared_slot = p >= L::EXT && p < L::EXT + L::EXT_SIZE;
  double s = 0.0, s2 = 0.0;
  if (p < L::P + 2) {
    const int per = (n_part + 3) / 4, lo = q * per, hi = lo + per < n_part ? lo + per : n_part;
    for (int k = lo; k < hi; ++k) s += (double)partials[(size_t)k * L::STRIDE + p];
    if (shared_slot) {
      for (int k = lo; k < hi; ++k) s2 += (double)partials[(size_t)k * L::STRIDE + L::EXT2 + (p - L::EXT)];
    }
  }
  s_sum[q][j] = s; s_sum2[q][j] = s2;
  __syncthreads();
  if (q == 0 && p < L::P + 2) {
    double total = (s_sum[0][j] + s_sum[1][j]) + (s_sum[2][j] + s_sum[3][j]);
    if (shared_slot) total += (s_sum2[0][j] + s_sum2[1][j]) + (s_sum2[2][j] + s_sum2[3][j]);
    if (p < L::P) {
      grad[p] = p < L::A ? (float)total - ent_coef : (float)total;
    } else {
      stats[p - L::P] = (float)(total / (double)batch);
      if (p == L::P) {
        float ent = 0.0f;
        for (int k = 0; k < L::A; ++k) ent += (0.5f + TB_LN_SQRT_2PI) + params[L::LOG_STD + k];
        stats[2] = ent;
      }
    }
  }
}

}  // namespace

// rex_learner_rnn.h -- the policy loss of the reference's RECURRENT agent (networks.py:113-159: O -> F -> GRU(100) -> A) over the episode memory and
// its nine parameter gradients by backpropagation through time, as kernels (rex_ppo_recurrent_policy_loss).  fp32 throughout; sigmoid and
// tanh from expf / tanhf.  Formulas: include/rexsim.h.  Every sum runs in a fixed order, no atomics: two calls return the same bits.
// The loss head, the MFMA block, the row length and the workgroup sum are rex_learner.h's helpers; the entry point is in rex_learner.hip.
//
// Decomposition.  Wg = [Wgx | Wgh], Wc = [Wcx | Wch].  Whatever does not depend on the recurrence is a product over 64-step tiles of one
// episode row (tiles wholly beyond the row's length are skipped, steps beyond it masked); only the H x 3H part is a scan over t.
//   pack      Wgh, Wch -> [k][j] and [j][k] copies for the scans; Wgx, Wcx, bg, bc -> zero-padded [384][Fp], its transpose, [384]
//   input     x = relu(W1 o + b1), a compensated fp32 dot product   -> X [n][Fp]
//   rows      ACT [n][384] = X Wx^T + b           v_mfma_f32_32x32x2_f32, a wave owns 64 steps x 32 units, operands straight from L2
//   scan fwd  a workgroup of 512 threads owns 8 rows; Wh^T (30 000 floats) resident in LDS; per step: gates (thread = unit x 4 rows),
//             barrier, candidate and h (thread = unit x 2 rows), barrier.  ACT <- r, u, c; HS <- h_t; RH <- r h_{t-1}
//   head      one thread per valid step: m = tanh(Wm h + bm), the step's KL and ratio . advantage
//   rowsum    one workgroup per row: kl_row, the row's loss term; loss: one workgroup adds the rows
//   -- with gradients --
//   head      the seeds g_z, g_l of every valid step (w_r from kl_row)  -> GZL [n][16]
//   scan bwd  the reverse recurrence of rexsim.h, Wh [j][k] resident in LDS, the carry in registers; three barriers per step.
//             ACT <- da_r, da_u, da_c
//   wgrad     dWg, dWc = ACT^T [X | h_{t-1} or r h_{t-1}]   MFMA, K = the steps, split over up to 64 groups of tiles -> partials
//   rows'     dx = ACT Wx, da1 = dx [x > 0]                 MFMA, overwrites X
//   outer     the thin products dW1 = da1^T o, dWm = g_z^T h and the column sums db1, dbg, dbc, dbm, dlogstd: one thread per column,
//             up to 512 groups of tiles -> partials
//   final     every gradient element = its partials added in index order, written in torch layout
// The loop bound of a scan is the largest length of the workgroup's rows, the same for every thread; rows are masked one by one, so every
// barrier is reached by the whole workgroup.  8 rows per workgroup: at 4 096 rows that is 512 workgroups (two rounds of one per CU, the
// LDS-resident weights allow no more), at 25 rows four, where the per-step latency -- two or three barriers and 300 LDS-fed FMAs per
// thread -- sets the time, not the row count.
//
// Workspace (the caller's): per memory slot (one step of one row) Fp + 384 + 128 + 128 + 16 + 2 floats -- X, ACT, HS, RH, GZL, the two
// loss terms -- with Fp = hidden1 rounded up to 32: 882 floats = 3 528 bytes at hidden1 = 200; plus the packed weights and the partials,
// which do not grow with the memory (rnn_workspace below).
#pragma once
#include "rex_learner.h"

namespace rex {

#define REX_RNN_H 100               /* the GRU's state (tf.contrib.rnn.GRUBlockCell(100)) */
#define REX_RNN_HP 128              /* a gate's block of ACT, the row stride of HS and RH */
#define REX_RNN_GP 384              /* ACT's row stride: r | u | c */
#define REX_RNN_ROWS 8              /* episode rows of a scan workgroup */
#define REX_RNN_SCAN_THREADS 512
#define REX_RNN_KSPLIT 64           /* groups of tiles of the weight-gradient product */
#define REX_RNN_OSPLIT 512          /* groups of tiles of the thin products */

struct RnnWs { size_t wht, wh, wxp, wxt, biasp, x, act, hs, rh, gzl, klt, sat, rowloss, pw, pb, pm, pz, p1, total; int Fp, ntiles, ksplit, osplit; };
__host__ __device__ __forceinline__ RnnWs rnn_workspace(int R, int T, int O, int F) {
  RnnWs w;
  const size_t H = REX_RNN_H, HP = REX_RNN_HP, GP = REX_RNN_GP, N = (size_t)R * T;
  w.Fp = ppo_up(F, 32);
  const size_t Fp = w.Fp;
  w.ntiles = (T + REX_PPO_TILE - 1) / REX_PPO_TILE;
  const size_t tiles = (size_t)R * w.ntiles;
  w.ksplit = tiles < REX_RNN_KSPLIT ? (int)tiles : REX_RNN_KSPLIT;
  w.osplit = tiles < REX_RNN_OSPLIT ? (int)tiles : REX_RNN_OSPLIT;
  size_t at = 0;
  auto take = [&](size_t n) { const size_t o = at; at += (n + 3) & ~(size_t)3; return o; };
  w.wht = take(3 * H * H); w.wh = take(3 * H * H); w.wxp = take(GP * Fp); w.wxt = take(Fp * GP); w.biasp = take(GP);
  w.x = take(N * Fp); w.act = take(N * GP); w.hs = take(N * HP); w.rh = take(N * HP); w.gzl = take(N * 16); w.klt = take(N); w.sat = take(N);
  w.rowloss = take(R);
  w.pw = take((size_t)w.ksplit * GP * (Fp + HP)); w.pb = take((size_t)w.osplit * GP); w.pm = take((size_t)w.osplit * 9 * H);
  w.pz = take((size_t)w.osplit * 16); w.p1 = take((size_t)w.osplit * (O + 1) * Fp);
  w.total = at;
  return w;
}
__host__ __device__ __forceinline__ int rnn_scan_lds_floats() { return 3 * REX_RNN_H * REX_RNN_H + 4 * REX_RNN_H * REX_RNN_ROWS; }

struct RnnArgs {
  const float *w1, *b1, *wg, *bg, *wc, *bc, *wm, *bm, *logstd;        // the network, torch layout
  const float *observ, *action, *old_mean, *old_logstd, *advantage;   // [R][T][O], [R][T][A] x 3, [R][T]
  const int32_t* length;
  float *wht, *wh, *wxp, *wxt, *biasp, *x, *act, *hs, *rh, *gzl, *klt, *sat, *rowloss, *pw, *pb, *pm, *pz, *p1;
  float* kl_row;
  int O, A, F, Fp, R, T, NT, ksplit, osplit;
  float penalty, cutoff, coef, inv_rt;
};
struct RnnGradDev { float *w1, *b1, *wg, *bg, *wc, *bc, *wm, *bm, *logstd; };

// the tile's row, first step and number of valid steps (0: skip it)
__device__ __forceinline__ int rnn_tile(const RnnArgs& p, int tile, size_t* base) {
  const int r = tile / p.NT, t0 = (tile - r * p.NT) * REX_PPO_TILE;
  const int len = ppo_row_len(p.length, r, p.T);
  *base = (size_t)r * p.T + t0;
  return t0 >= len ? 0 : min(REX_PPO_TILE, len - t0);
}
// column of ACT of gate unit j (torch order: r 0..99, u 100..199, c 200..299)
__host__ __device__ __forceinline__ int rnn_col(int j) { return REX_RNN_HP * (j / REX_RNN_H) + j % REX_RNN_H; }

__global__ void rex_rnn_pack_kernel(RnnArgs p) {
  const int H = REX_RNN_H, F = p.F, Fp = p.Fp, ld = F + H;
  const int nx = REX_RNN_GP * Fp, total = nx > 3 * H * H ? nx : 3 * H * H;
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
    if (t < 3 * H * H) {
      const int j = t / H, k = t - j * H;
      const float v = j < 2 * H ? p.wg[(size_t)j * ld + F + k] : p.wc[(size_t)(j - 2 * H) * ld + F + k];
      p.wh[t] = v;
      p.wht[k * 3 * H + j] = v;
    }
    if (t >= nx) continue;
    const int jp = t / Fp, f = t - jp * Fp, b = jp / REX_RNN_HP, u = jp - b * REX_RNN_HP;
    float v = 0.0f;
    if (u < H && f < F) v = b < 2 ? p.wg[(size_t)(b * H + u) * ld + f] : p.wc[(size_t)u * ld + f];
    p.wxp[t] = v;
    p.wxt[(size_t)f * REX_RNN_GP + jp] = v;
    if (t < REX_RNN_GP) {
      const int bb = t / REX_RNN_HP, uu = t - bb * REX_RNN_HP;
      p.biasp[t] = uu < H ? (bb < 2 ? p.bg[bb * H + uu] : p.bc[uu]) : 0.0f;
    }
  }
}

// x = relu(W1 o + b1), zero in the padded columns; one thread per (valid step, column)
__global__ __launch_bounds__(256) void rex_rnn_input_kernel(RnnArgs p) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t n = idx / p.Fp;
  if (n >= (size_t)p.R * p.T) return;
  const int f = (int)(idx - n * p.Fp), r = (int)(n / p.T), t = (int)(n - (size_t)r * p.T);
  if (t >= ppo_row_len(p.length, r, p.T)) return;
  float acc = 0.0f;
  if (f < p.F) {
    // a compensated dot product (Ogita, Rump, Oishi: Dot2 -- every product's and every sum's rounding error carried along in fp32): the
    // ReLU's branch, which the backward pass takes again as [x > 0], is decided as the exactly evaluated sum decides it whenever that sum
    // is representable at all; a plain fp32 chain of 22 terms of order 1 places a pre-activation of 1e-8 on either side of the kink
    float hi = p.b1[f], lo = 0.0f;
    for (int o = 0; o < p.O; ++o) {
      const float w = p.w1[f * p.O + o], x = p.observ[n * p.O + o];
      const float h = w * x;
      const float r = fmaf(w, x, -h);
      const float q = hi + h;
      const float z = q - hi;
      const float e = (hi - (q - z)) + (h - z);
      hi = q;
      lo += e + r;
    }
    acc = fmaxf(hi + lo, 0.0f);
  }
  p.x[idx] = acc;
}

// D[step][unit] = sum_k A[step][k] W[unit][k] over one tile: !BWD: ACT = X Wxp^T + bias; BWD: X <- (ACT Wxt^T) [X > 0].
// A wave owns unit tiles wave, wave + 4, ...; a lane's four consecutive k are one 16-byte read in both operands (k order as in rex_learner.h).
template <bool BWD>
__global__ __launch_bounds__(256) void rex_rnn_rows_kernel(RnnArgs p) {
  size_t base;
  const int nvalid = rnn_tile(p, blockIdx.x, &base);
  if (nvalid == 0) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r32 = lane & 31, hh = lane >> 5;
  const int K = BWD ? REX_RNN_GP : p.Fp, NU = (BWD ? p.Fp : REX_RNN_GP) / 32;
  const float* A = BWD ? p.act : p.x;
  const float* W = BWD ? p.wxt : p.wxp;
  // (steps beyond the row's length read its last valid step: in bounds, their results are dropped)
  const float4* a0 = reinterpret_cast<const float4*>(A + (base + min(r32, nvalid - 1)) * K + 4 * hh);
  const float4* a1 = reinterpret_cast<const float4*>(A + (base + min(32 + r32, nvalid - 1)) * K + 4 * hh);
  for (int ut = wave; ut < NU; ut += 4) {
    const float4* bw = reinterpret_cast<const float4*>(W + (size_t)(32 * ut + r32) * K + 4 * hh);
    ppo_f16 acc[2];
#pragma unroll
    for (int e = 0; e < 16; ++e) { acc[0][e] = 0.0f; acc[1][e] = 0.0f; }
#pragma unroll 4
    for (int g = 0; g < K / 8; ++g) {
      const float4 x0 = a0[2 * g], x1 = a1[2 * g], b = bw[2 * g];
      ppo_mfma_k4(acc[0], acc[1], x0, x1, b);
    }
    const int col = 32 * ut + r32;
    const float bias = BWD ? 0.0f : p.biasp[col];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int s = 32 * mt + ppo_acc_row(e, hh);
        if (s < nvalid) {
          if constexpr (!BWD) p.act[(base + s) * REX_RNN_GP + col] = acc[mt][e] + bias;
          else { float* xp = p.x + (base + s) * p.Fp + col; *xp = *xp > 0.0f ? acc[mt][e] : 0.0f; }
        }
      }
  }
}

// the forward recurrence of 8 rows.  LDS: wt [k][300] (unit j of torch order), hs / rhs / us [unit][8 rows]
__global__ __launch_bounds__(REX_RNN_SCAN_THREADS) void rex_rnn_scan_fwd_kernel(RnnArgs p) {
  extern __shared__ __attribute__((aligned(16))) float rnn_lds[];
  __shared__ int lens[REX_RNN_ROWS];
  const int H = REX_RNN_H, G = REX_RNN_ROWS, tid = threadIdx.x, r0 = blockIdx.x * G, T = p.T;
  float* wt = rnn_lds;
  float* hs = wt + 3 * H * H;
  float* rhs = hs + H * G;
  float* us = rhs + H * G;
  for (int i = tid; i < 3 * H * H; i += REX_RNN_SCAN_THREADS) wt[i] = p.wht[i];
  for (int i = tid; i < 3 * H * G; i += REX_RNN_SCAN_THREADS) hs[i] = 0.0f;
  if (tid < G) lens[tid] = r0 + tid < p.R ? ppo_row_len(p.length, r0 + tid, T) : 0;
  __syncthreads();
  int lmax = 0;
#pragma unroll
  for (int i = 0; i < G; ++i) lmax = max(lmax, lens[i]);
  const int jA = tid & 255, halfA = tid >> 8, colA = rnn_col(jA < 2 * H ? jA : 0);
  const int jB = tid & 127, qB = tid >> 7;
  int lenA[4], lenB[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) lenA[i] = lens[4 * halfA + i];
#pragma unroll
  for (int i = 0; i < 2; ++i) lenB[i] = lens[2 * qB + i];
  const float4* hs4 = reinterpret_cast<const float4*>(hs);
  const float2* rhs2 = reinterpret_cast<const float2*>(rhs);
  for (int t = 0; t < lmax; ++t) {              // (lmax: the same for every thread of the workgroup)
    if (jA < 2 * H) {                           // r and u of unit jA for rows 4 halfA ..
      float gx[4], acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int i = 0; i < 4; ++i) gx[i] = t < lenA[i] ? p.act[((size_t)(r0 + 4 * halfA + i) * T + t) * REX_RNN_GP + colA] : 0.0f;
#pragma unroll 4
      for (int k = 0; k < H; ++k) {
        const float w = wt[k * 3 * H + jA];
        const float4 h = hs4[k * 2 + halfA];
        acc[0] = fmaf(w, h.x, acc[0]); acc[1] = fmaf(w, h.y, acc[1]); acc[2] = fmaf(w, h.z, acc[2]); acc[3] = fmaf(w, h.w, acc[3]);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (t < lenA[i]) {
          const int row = 4 * halfA + i;
          const size_t n = (size_t)(r0 + row) * T + t;
          const float g = 1.0f / (1.0f + expf(-(acc[i] + gx[i])));
          p.act[n * REX_RNN_GP + colA] = g;
          if (jA < H) {
            const float rh = g * hs[jA * G + row];
            rhs[jA * G + row] = rh;
            p.rh[n * REX_RNN_HP + jA] = rh;
          } else us[(jA - H) * G + row] = g;
        }
    }
    __syncthreads();
    if (jB < H) {                               // c and h of unit jB for rows 2 qB, 2 qB + 1
      float gx[2], acc[2] = {0.0f, 0.0f};
#pragma unroll
      for (int i = 0; i < 2; ++i) gx[i] = t < lenB[i] ? p.act[((size_t)(r0 + 2 * qB + i) * T + t) * REX_RNN_GP + 2 * REX_RNN_HP + jB] : 0.0f;
#pragma unroll 4
      for (int k = 0; k < H; ++k) {
        const float w = wt[k * 3 * H + 2 * H + jB];
        const float2 rh = rhs2[k * 4 + qB];
        acc[0] = fmaf(w, rh.x, acc[0]); acc[1] = fmaf(w, rh.y, acc[1]);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
        if (t < lenB[i]) {
          const int row = 2 * qB + i;
          const size_t n = (size_t)(r0 + row) * T + t;
          const float c = tanhf(acc[i] + gx[i]), u = us[jB * G + row], h = hs[jB * G + row];
          const float hn = u * h + (1.0f - u) * c;
          hs[jB * G + row] = hn;
          p.act[n * REX_RNN_GP + 2 * REX_RNN_HP + jB] = c;
          p.hs[n * REX_RNN_HP + jB] = hn;
        }
    }
    __syncthreads();
  }
}

// one thread per valid step: the mean, the loss terms (!BWD) or the seeds (BWD): the loss head of rex_learner.h on a register z
template <bool BWD>
__global__ __launch_bounds__(256) void rex_rnn_head_kernel(RnnArgs p) {
  const size_t n = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= (size_t)p.R * p.T) return;
  const int r = (int)(n / p.T), t = (int)(n - (size_t)r * p.T), A = p.A;
  if (t >= ppo_row_len(p.length, r, p.T)) return;
  float z[REX_PPO_MAX_A];
#pragma unroll
  for (int a = 0; a < REX_PPO_MAX_A; ++a) z[a] = a < A ? p.bm[a] : 0.0f;
  const float4* h4 = reinterpret_cast<const float4*>(p.hs + n * REX_RNN_HP);
  for (int q = 0; q < REX_RNN_H / 4; ++q) {
    const float4 h = h4[q];
#pragma unroll
    for (int a = 0; a < REX_PPO_MAX_A; ++a)
      if (a < A) {
        const float* w = p.wm + a * REX_RNN_H + 4 * q;
        z[a] = fmaf(w[0], h.x, z[a]); z[a] = fmaf(w[1], h.y, z[a]); z[a] = fmaf(w[2], h.z, z[a]); z[a] = fmaf(w[3], h.w, z[a]);
      }
  }
  PpoGauss h;
  ppo_gauss_terms(h, z, A, true, p.logstd, p.old_logstd, p.old_mean, p.action, n * A);
  const float kl = h.kl;
  const float ra = h.ratio * p.advantage[n];
  if constexpr (!BWD) {
    p.klt[n] = kl;
    p.sat[n] = ra;
  } else {
    const float wr = ppo_row_weight(p.kl_row[r], p.penalty, p.cutoff, p.coef);
    float out[16];
#pragma unroll
    for (int a = 0; a < REX_PPO_MAX_A; ++a) {
      float gz, gl;
      ppo_gauss_seed(h, a, wr, ra, p.inv_rt, &gz, &gl);
      out[a] = a < A ? gz : 0.0f;
      out[8 + a] = a < A ? gl : 0.0f;
    }
    float4* o4 = reinterpret_cast<float4*>(p.gzl + n * 16);
#pragma unroll
    for (int q = 0; q < 4; ++q) o4[q] = make_float4(out[4 * q], out[4 * q + 1], out[4 * q + 2], out[4 * q + 3]);
  }
}

// one workgroup per row: its steps' terms, a thread's in step order, then a tree -> kl_row, the row's loss term
__global__ __launch_bounds__(REX_PPO_THREADS) void rex_rnn_rowsum_kernel(RnnArgs p, float* __restrict__ kl_row) {
  const int tid = threadIdx.x, r = blockIdx.x, len = ppo_row_len(p.length, r, p.T);
  float a = 0.0f, b = 0.0f;
  for (int t = tid; t < len; t += REX_PPO_THREADS) { a += p.klt[(size_t)r * p.T + t]; b += p.sat[(size_t)r * p.T + t]; }
  const float* ra = ppo_block_sum<0>(tid, a);
  const float* rb = ppo_block_sum<1>(tid, b);
  if (tid == 0) {
    float kl;
    const float term = ppo_row_loss(ra[0], rb[0], p.T, p.penalty, p.cutoff, p.coef, &kl);
    kl_row[r] = kl;
    p.rowloss[r] = term;
  }
}
__global__ __launch_bounds__(REX_PPO_THREADS) void rex_rnn_loss_kernel(RnnArgs p, float* __restrict__ loss) {
  const int tid = threadIdx.x;
  float acc = 0.0f;
  for (int r = tid; r < p.R; r += REX_PPO_THREADS) acc += p.rowloss[r];
  const float* red = ppo_block_sum(tid, acc);
  if (tid == 0) *loss = red[0] / (float)p.R;
}

// the reverse recurrence of 8 rows.  LDS: w [300][k], wm [8][k], dac [100][8 rows], dag [200][8 rows].  Thread (k, rows 2 q, 2 q + 1)
// keeps its two carries in registers; the next step's activations are read while this step's products run.
__global__ __launch_bounds__(REX_RNN_SCAN_THREADS) void rex_rnn_scan_bwd_kernel(RnnArgs p) {
  extern __shared__ __attribute__((aligned(16))) float rnn_lds[];
  __shared__ int lens[REX_RNN_ROWS];
  __shared__ float wms[REX_PPO_MAX_A * REX_RNN_H];
  const int H = REX_RNN_H, G = REX_RNN_ROWS, tid = threadIdx.x, r0 = blockIdx.x * G, T = p.T, A = p.A;
  float* w = rnn_lds;
  float* dac = w + 3 * H * H;
  float* dag = dac + H * G;
  for (int i = tid; i < 3 * H * H; i += REX_RNN_SCAN_THREADS) w[i] = p.wh[i];
  for (int i = tid; i < REX_PPO_MAX_A * H; i += REX_RNN_SCAN_THREADS) wms[i] = i < A * H ? p.wm[i] : 0.0f;
  if (tid < G) lens[tid] = r0 + tid < p.R ? ppo_row_len(p.length, r0 + tid, T) : 0;
  __syncthreads();
  int lmax = 0;
#pragma unroll
  for (int i = 0; i < G; ++i) lmax = max(lmax, lens[i]);
  const int k = tid & 127, q = tid >> 7;
  const bool on = k < H;
  int len[2];
  size_t row0[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) { len[i] = on ? lens[2 * q + i] : 0; row0[i] = (size_t)(r0 + 2 * q + i) * T; }
  const float2* dac2 = reinterpret_cast<const float2*>(dac);
  const float2* dag2 = reinterpret_cast<const float2*>(dag);
  float carry[2] = {0.0f, 0.0f};
  float cr[2], cu[2], cc[2], chp[2], cdz[2];    // this step's r, u, c, h_{t-1}, Wm^T g_z
  auto fetch = [&](int t, int i) {
    cr[i] = cu[i] = cc[i] = chp[i] = cdz[i] = 0.0f;
    if (t >= 0 && t < len[i]) {
      const size_t n = row0[i] + t;
      const float* a = p.act + n * REX_RNN_GP + k;
      cr[i] = a[0]; cu[i] = a[REX_RNN_HP]; cc[i] = a[2 * REX_RNN_HP];
      chp[i] = t > 0 ? p.hs[(n - 1) * REX_RNN_HP + k] : 0.0f;
      float d = 0.0f;
      for (int a2 = 0; a2 < A; ++a2) d = fmaf(wms[a2 * H + k], p.gzl[n * 16 + a2], d);
      cdz[i] = d;
    }
  };
  fetch(lmax - 1, 0); fetch(lmax - 1, 1);
  for (int t = lmax - 1; t >= 0; --t) {         // (lmax: the same for every thread of the workgroup)
    float r[2], hp[2];
    bool act[2];
    if (on) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int row = 2 * q + i;
        act[i] = t < len[i];
        r[i] = cr[i]; hp[i] = chp[i];
        float dacv = 0.0f, dau = 0.0f;
        if (act[i]) {
          const float u = cu[i], c = cc[i], dh = cdz[i] + carry[i];
          const float du = dh * (hp[i] - c), dc = dh * (1.0f - u);
          carry[i] = dh * u;
          dacv = dc * (1.0f - c * c);
          dau = du * u * (1.0f - u);
          float* a = p.act + (row0[i] + t) * REX_RNN_GP + k;
          a[REX_RNN_HP] = dau; a[2 * REX_RNN_HP] = dacv;
        }
        dac[k * G + row] = dacv;
        dag[(H + k) * G + row] = dau;
      }
    }
    __syncthreads();
    if (on) {                                   // drh = Wch^T da_c
      float acc[2] = {0.0f, 0.0f};
#pragma unroll 4
      for (int j = 0; j < H; ++j) {
        const float wv = w[(2 * H + j) * H + k];
        const float2 d = dac2[j * 4 + q];
        acc[0] = fmaf(wv, d.x, acc[0]); acc[1] = fmaf(wv, d.y, acc[1]);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        float dar = 0.0f;
        if (act[i]) {
          carry[i] = fmaf(acc[i], r[i], carry[i]);
          dar = acc[i] * hp[i] * r[i] * (1.0f - r[i]);
          p.act[(row0[i] + t) * REX_RNN_GP + k] = dar;
        }
        dag[k * G + 2 * q + i] = dar;
      }
    }
    __syncthreads();
    if (on) {                                   // dhg = Wgh^T da_g
      fetch(t - 1, 0); fetch(t - 1, 1);
      float acc[2] = {0.0f, 0.0f};
#pragma unroll 4
      for (int j = 0; j < 2 * H; ++j) {
        const float wv = w[j * H + k];
        const float2 d = dag2[j * 4 + q];
        acc[0] = fmaf(wv, d.x, acc[0]); acc[1] = fmaf(wv, d.y, acc[1]);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) if (act[i]) carry[i] += acc[i];
    }
    __syncthreads();
  }
}

// dWg, dWc: D[ACT column][input] = sum over steps of ACT[n][column] Z[n][input], Z = [X | h_{t-1} (r, u) or r h_{t-1} (c)].
// A wave owns 64 ACT columns x 32 inputs; grid.y = the group of tiles (tile = group, group + ksplit, ...); partials [group][384][Fp + 128].
__global__ __launch_bounds__(256) void rex_rnn_wgrad_kernel(RnnArgs p) {
  const int lane = threadIdx.x & 63, r32 = lane & 31, hh = lane >> 5;
  const int NI = (p.Fp + REX_RNN_HP) / 32, gw = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (gw >= 6 * NI) return;                     // (whole waves; no barrier below)
  const int jt = gw / NI, it = gw - jt * NI, j0 = 64 * jt, i0 = 32 * it, Fp = p.Fp, tiles = p.R * p.NT;
  const bool zx = i0 < Fp, zh = jt < 4;
  const int kk = i0 - Fp + r32;
  ppo_f16 acc[2];
#pragma unroll
  for (int e = 0; e < 16; ++e) { acc[0][e] = 0.0f; acc[1][e] = 0.0f; }
  for (int tile = blockIdx.y; tile < tiles; tile += p.ksplit) {
    size_t base;
    const int nvalid = rnn_tile(p, tile, &base);
    const bool first = (tile % p.NT) == 0;
#pragma unroll 4
    for (int s2 = 0; s2 < nvalid; s2 += 2) {
      const int s = s2 + hh;
      const bool valid = s < nvalid;
      const size_t n = base + s;
      float a0 = 0.0f, a1 = 0.0f, b = 0.0f;
      if (valid) {
        a0 = p.act[n * REX_RNN_GP + j0 + r32]; a1 = p.act[n * REX_RNN_GP + j0 + 32 + r32];
        if (zx) b = p.x[n * Fp + i0 + r32];
        else if (!zh) b = p.rh[n * REX_RNN_HP + kk];
        else if (!(first && s == 0)) b = p.hs[(n - 1) * REX_RNN_HP + kk];
      }
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b, acc[1], 0, 0, 0);
    }
  }
  const int ldp = Fp + REX_RNN_HP;
  float* pw = p.pw + (size_t)blockIdx.y * REX_RNN_GP * ldp;
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int e = 0; e < 16; ++e) pw[(size_t)(j0 + 32 * mt + ppo_acc_row(e, hh)) * ldp + i0 + r32] = acc[mt][e];
}

// the thin products: out[c][k] = sum over steps of S[n][c] V[n][k] (c < C) and out[C][k] = sum V[n][k]; one thread per column k,
// grid.y = the group of tiles; partials [group][C + 1][Kp]
template <int C>
__global__ __launch_bounds__(128) void rex_rnn_outer_kernel(RnnArgs p, const float* __restrict__ S, int lds, const float* __restrict__ V, int ldv, int Kp,
                                                            float* __restrict__ part) {
  const int k = blockIdx.x * 128 + threadIdx.x, tiles = p.R * p.NT;
  if (k >= Kp) return;
  float acc[C + 1];
#pragma unroll
  for (int c = 0; c <= C; ++c) acc[c] = 0.0f;
  for (int tile = blockIdx.y; tile < tiles; tile += p.osplit) {
    size_t base;
    const int nvalid = rnn_tile(p, tile, &base);
    for (int s = 0; s < nvalid; ++s) {
      const size_t n = base + s;
      const float v = V[n * ldv + k];
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] = fmaf(S[n * lds + c], v, acc[c]);
      acc[C] += v;
    }
  }
#pragma unroll
  for (int c = 0; c <= C; ++c) part[((size_t)blockIdx.y * (C + 1) + c) * Kp + k] = acc[c];
}

// every gradient element: its partials added in group order, written in torch layout
__global__ __launch_bounds__(256) void rex_rnn_final_kernel(RnnArgs p, RnnGradDev g) {
  const int H = REX_RNN_H, F = p.F, O = p.O, A = p.A, Fp = p.Fp, ld = F + H, ldp = Fp + REX_RNN_HP;
  const int nw1 = F * O, nwg = 2 * H * ld, nwc = H * ld, nwm = A * H;
  int k = blockIdx.x * 256 + threadIdx.x;
  const float* src; size_t stride; int count; float* dst;
  if (k < nw1) { const int f = k / O, o = k - f * O; src = p.p1 + (size_t)o * Fp + f; stride = (size_t)(O + 1) * Fp; count = p.osplit; dst = g.w1 + k; }
  else if ((k -= nw1) < F) { src = p.p1 + (size_t)O * Fp + k; stride = (size_t)(O + 1) * Fp; count = p.osplit; dst = g.b1 + k; }
  else if ((k -= F) < nwg + nwc) {
    const bool gate = k < nwg;
    const int kk = gate ? k : k - nwg, j = kk / ld, col = kk - j * ld;
    src = p.pw + (size_t)rnn_col(gate ? j : 2 * H + j) * ldp + (col < F ? col : Fp + col - F); stride = (size_t)REX_RNN_GP * ldp; count = p.ksplit;
    dst = (gate ? g.wg : g.wc) + kk;
  }
  else if ((k -= nwg + nwc) < 3 * H) { src = p.pb + rnn_col(k); stride = REX_RNN_GP; count = p.osplit; dst = k < 2 * H ? g.bg + k : g.bc + (k - 2 * H); }
  else if ((k -= 3 * H) < nwm) { src = p.pm + k; stride = 9 * H; count = p.osplit; dst = g.wm + k; }
  else if ((k -= nwm) < A) { src = p.pz + k; stride = 16; count = p.osplit; dst = g.bm + k; }
  else if ((k -= A) < A) { src = p.pz + 8 + k; stride = 16; count = p.osplit; dst = g.logstd + k; }
  else return;
  float acc = 0.0f;
  for (int b = 0; b < count; ++b) acc += src[(size_t)b * stride];
  *dst = acc;
}

}  // namespace rex

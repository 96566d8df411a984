// rex_learner.h -- the LEARNER of the reference's PPO agents as fused kernels (rex_ppo_returns, rex_ppo_policy_loss, rex_ppo_value_loss):
// what one epoch of `_update_policy` / `_update_value` (agents/ppo/algorithm.py:289-301, 376-434) computes -- the loss of a ForwardGaussianPolicy
// network (networks.py:69-112: O -> H1 -> H2 -> A, two ReLU layers) over the episode memory and its parameter gradients -- in ONE pass over the
// memory: the activations of a tile of samples live in LDS, the 200 x 100 products run on the matrix cores, padded steps are skipped.
// fp32 throughout.  Formulas and layouts: include/rexsim.h.
//
// Mapping.  The memory is cut into TILES of 64 consecutive steps of one episode row; tiles wholly beyond the row's length are skipped.  A
// workgroup of four waves walks tiles (its index, + the grid size, ...) and for each:
//   1  x [64][O] -> LDS (zero beyond the row's length: a padded slot is never read)
//   2  h1 = relu(W1 x + b1)            one thread per unit, its row of W1 in registers
//   3  h2 = relu(W2 h1 + b2)           v_mfma_f32_32x32x2_f32: wave w owns units 32 w .. 32 w + 31, both halves of the tile
//   4  z = W3 h2 + b3                  one thread per (sample, output pair)
//   5  the loss terms of the tile's samples and the seeds g_z of the backward pass (wave 0, one lane per sample): ppo_gauss_terms / _seed
//   6  dh2 = W3^T g_z . relu', dW3 += g_z^T h2, db2 += sum dh2    one thread per (unit, half tile); dh2 overwrites h2
//   7  dW2 += dh2^T h1                 MFMA, K = the 64 samples; wave w owns input units 32 w .. and 32 (w + 4) .., 8 accumulator tiles
//   8  dh1 = dh2 W2 . relu'            MFMA, K = H2; overwrites h1
//   9  dW1 += dh1^T x, db1 += sum dh1  one thread per unit
// The partial gradients stay in registers over all the tiles of the workgroup and are written ONCE to the workspace; rex_ppo_reduce_kernel
// adds the workgroups' partials in index order.  Every sum has a fixed order: the result does not depend on timing.
// W2 does not fit LDS next to the activations (64 x 260 + 64 x 132 floats): the two MFMA products that read it take it from L2, four
// 16-byte reads in flight per lane, out of two zero-padded copies the pack kernel writes in front of every call -- [H2p][H1p] for step 3,
// its transpose [H1p][H2p] for step 8 -- so that a lane's four consecutive k are one read in both.  The k order inside a group of 8 is
// permuted the same way for both operands (lane half h takes k = 8 g + 4 h + c at MFMA c of the group).
//
// Shared with rex_learner_rnn.h (one copy each): the Gaussian-policy loss head -- ppo_gauss_terms, ppo_gauss_seed, ppo_row_weight, ppo_row_loss --
// the four-k MFMA block ppo_mfma_k4, ppo_row_len and the workgroup sum ppo_block_sum.  The build fixes arithmetic by source (-ffp-contract=on):
// an expression moved into one of them keeps its spelling and with it every rounding.  The C ABI of both learners: rex_learner.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rex {

#define REX_PPO_TILE 64
#define REX_PPO_THREADS 256
#define REX_PPO_MAX_GROUPS 256      /* workgroups of a launch = partial-gradient blocks of the workspace */
#define REX_PPO_MAX_H1 256
#define REX_PPO_MAX_H2 128
#define REX_PPO_MAX_A 8

typedef float ppo_f16 __attribute__((ext_vector_type(16)));

__host__ __device__ __forceinline__ int ppo_up(int n, int m) { return (n + m - 1) / m * m; }

// float offsets of a network's parameters inside a partial-gradient block: torch order and torch layout ([out][in])
struct PpoOff { int w1, b1, w2, b2, w3, b3, logstd, total; };
__host__ __device__ __forceinline__ PpoOff ppo_offsets(int O, int A, int H1, int H2) {
  PpoOff o;
  o.w1 = 0; o.b1 = o.w1 + H1 * O; o.w2 = o.b1 + H1; o.b2 = o.w2 + H2 * H1; o.w3 = o.b2 + H2; o.b3 = o.w3 + A * H2; o.logstd = o.b3 + A;
  o.total = ppo_up(o.logstd + A, 4);
  return o;
}
// float offsets of the caller's workspace: the two packed copies of W2, the per-tile loss terms [2][R NT], the partial gradients [G][total]
struct PpoWs { size_t w2p, w2t, part, pgrad, total; int groups, ntiles; };
__host__ __device__ __forceinline__ PpoWs ppo_workspace(int R, int T, int O, int A, int H1, int H2) {
  PpoWs w;
  const size_t H1p = ppo_up(H1, 32), H2p = ppo_up(H2, 32);
  w.ntiles = (T + REX_PPO_TILE - 1) / REX_PPO_TILE;
  const size_t tiles = (size_t)R * w.ntiles;
  w.groups = tiles < REX_PPO_MAX_GROUPS ? (int)tiles : REX_PPO_MAX_GROUPS;
  w.w2p = 0; w.w2t = w.w2p + H1p * H2p; w.part = w.w2t + H1p * H2p;
  w.pgrad = w.part + ((2 * tiles + 3) & ~(size_t)3);
  w.total = w.pgrad + (size_t)w.groups * ppo_offsets(O, A, H1, H2).total;
  return w;
}
__host__ __device__ __forceinline__ int ppo_lds_floats(int OP, int H1p, int H2p) {
  return REX_PPO_TILE * OP + REX_PPO_TILE * (H1p + 4) + REX_PPO_TILE * (H2p + 4) + REX_PPO_MAX_A * H2p + 4 * REX_PPO_MAX_A * REX_PPO_TILE;
}

struct PpoArgs {
  const float *w1, *b1, *b2, *w3, *b3, *logstd;            // the network, torch layout (W2 comes packed)
  const float *w2p, *w2t;
  const float *observ, *action, *old_mean, *old_logstd;    // [R][T][O], [R][T][A] x 3 (the value net reads observ only)
  const float* target;                                     // [R][T]: the normalised advantage (policy) or the return (value)
  const int32_t* length;                                   // [R]
  const float* kl_row;                                     // [R]: the backward pass of the policy reads it
  float* part;                                             // [2][R NT] per-tile sums: KL and ratio . advantage, or 0.5 (return - value)^2
  float* pgrad;                                            // [groups][ppo_offsets().total]
  float* value_out;                                        // [R][T] (value net, nullable)
  int O, A, H1, H2, H1p, H2p, R, T, NT;
  float penalty, cutoff, coef, inv_rt;
};

__device__ __forceinline__ float ppo_wave_sum(float v) {     // a fixed tree over the 64 lanes, every lane gets the total
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}
// the row of register e of lane half h in a 32 x 32 accumulator tile (the column is lane & 31)
__device__ __forceinline__ int ppo_acc_row(int e, int h) { return (e & 3) + 8 * (e >> 2) + 4 * h; }
// a row's length as every kernel reads it: inside [0, T]
__device__ __forceinline__ int ppo_row_len(const int32_t* length, int r, int T) { return min(max(length[r], 0), T); }
// four k of a product D[64][32] += A[64][k] B[32][k]: the two 32-row halves of A (x0, x1) against one B operand, k = the float4's lanes
__device__ __forceinline__ void ppo_mfma_k4(ppo_f16& acc0, ppo_f16& acc1, const float4& x0, const float4& x1, const float4& b) {
  acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(x0.x, b.x, acc0, 0, 0, 0); acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(x1.x, b.x, acc1, 0, 0, 0);
  acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(x0.y, b.y, acc0, 0, 0, 0); acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(x1.y, b.y, acc1, 0, 0, 0);
  acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(x0.z, b.z, acc0, 0, 0, 0); acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(x1.z, b.z, acc1, 0, 0, 0);
  acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(x0.w, b.w, acc0, 0, 0, 0); acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(x1.w, b.w, acc1, 0, 0, 0);
}
// the sum of the workgroup's REX_PPO_THREADS values v at [0] of the returned LDS slots: a halving tree, the same order in every kernel.
// A kernel with two sums gives each its own SLOT (its own 256 floats of LDS)
template <int SLOT = 0>
__device__ __forceinline__ const float* ppo_block_sum(int tid, float v) {
  __shared__ float red[REX_PPO_THREADS];
  red[tid] = v;
  __syncthreads();
  for (int m = REX_PPO_THREADS / 2; m >= 1; m >>= 1) {
    if (tid < m) red[tid] += red[tid + m];
    __syncthreads();
  }
  return red;
}

// ---- the Gaussian-policy loss head, shared with rex_learner_rnn.h: one sample's terms, its seeds, a row's weight and loss term ----
struct PpoGauss { float m[REX_PPO_MAX_A], dm[REX_PPO_MAX_A], dx[REX_PPO_MAX_A], ie2[REX_PPO_MAX_A], ev[REX_PPO_MAX_A], u2[REX_PPO_MAX_A], kl, ratio; };   // (ev = e^(2 l0 - 2 l) - 1)
// z [8]: the sample's pre-tanh means; at0: the float offset of its A actions in the [R][T][A] blocks; !valid: every term zero, nothing read
__device__ __forceinline__ void ppo_gauss_terms(PpoGauss& h, const float* z, int A, bool valid, const float* __restrict__ logstd, const float* __restrict__ old_logstd,
                                                const float* __restrict__ old_mean, const float* __restrict__ action, size_t at0) {
  float kl = 0.0f, dlp = 0.0f;
#pragma unroll
  for (int a = 0; a < REX_PPO_MAX_A; ++a) {
    h.m[a] = h.dm[a] = h.dx[a] = h.ie2[a] = h.ev[a] = h.u2[a] = 0.0f;
    if (a < A && valid) {
      const size_t at = at0 + a;
      const float l = logstd[a], l0 = old_logstd[at], m0 = old_mean[at], x = action[at];
      h.m[a] = tanhf(z[a]);
      h.dm[a] = h.m[a] - m0; h.dx[a] = x - h.m[a];
      h.ie2[a] = expf(-2.0f * l);
      // e^d - 1 and e^d - 1 - d of d = 2 l0 - 2 l without the cancellation of their terms (the KL of two close policies is the small
      // difference of numbers near 1): expm1f, and for small d the series d^2 / 2 (1 + d/3 (1 + d/4 (...)))
      const float d = 2.0f * l0 - 2.0f * l;
      h.ev[a] = expm1f(d);
      const float series = 0.5f * d * d * (1.0f + d * (1.0f / 3.0f) * (1.0f + d * 0.25f * (1.0f + d * 0.2f * (1.0f + d * (1.0f / 6.0f) * (1.0f + d * (1.0f / 7.0f) * (1.0f + d * 0.125f))))));
      const float phi = fabsf(d) < 0.25f ? series : h.ev[a] - d;
      const float u = h.dx[a] * expf(-l), u0 = (x - m0) * expf(-l0);
      h.u2[a] = u * u;
      kl += phi + h.dm[a] * h.dm[a] * h.ie2[a];
      dlp += -0.5f * (l - l0) - 0.5f * (h.u2[a] - u0 * u0);
    }
  }
  kl *= 0.5f;
  h.kl = kl;
  h.ratio = expf(dlp);
}
// the seeds of output a: d loss / d z_a and d loss / d logstd_a of the sample (ra = ratio . advantage)
__device__ __forceinline__ void ppo_gauss_seed(const PpoGauss& h, int a, float wr, float ra, float inv_rt, float* g_z, float* g_l) {
  const float dkl_dm = h.dm[a] * h.ie2[a], dkl_dl = -h.ev[a] - h.dm[a] * h.dm[a] * h.ie2[a];
  const float dlp_dm = h.dx[a] * h.ie2[a], dlp_dl = -0.5f + h.u2[a];
  const float gm = inv_rt * (wr * dkl_dm - ra * dlp_dm), gl = inv_rt * (wr * dkl_dl - ra * dlp_dl);
  *g_z = gm * (1.0f - h.m[a] * h.m[a]);
  *g_l = gl;
}
// w_r = d (row loss) / d kl_r
__device__ __forceinline__ float ppo_row_weight(float klr, float penalty, float cutoff, float coef) {
  return penalty + (klr > cutoff ? 2.0f * coef * (klr - cutoff) : 0.0f);
}
// a row's loss term surrogate + penalty kl + coef [kl > c] (kl - c)^2 from its sums of KL and ratio . advantage over the steps; *kl_out = kl_r
__device__ __forceinline__ float ppo_row_loss(float kl_sum, float sa_sum, int T, float penalty, float cutoff, float coef, float* kl_out) {
  const float kl = kl_sum / (float)T, surrogate = -(sa_sum / (float)T);
  const float over = kl - cutoff;
  const float cut = kl > cutoff ? coef * (over * over) : 0.0f;
  *kl_out = kl;
  return surrogate + penalty * kl + cut;
}

// W2 [H2][H1] (torch) -> w2p [H2p][H1p] and w2t [H1p][H2p], zero beyond the layer's widths
__global__ void rex_ppo_pack_kernel(const float* __restrict__ w2, int H1, int H2, int H1p, int H2p, float* __restrict__ w2p, float* __restrict__ w2t) {
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < H1p * H2p; t += gridDim.x * blockDim.x) {
    const int j = t / H1p, i = t - j * H1p;
    const float v = (j < H2 && i < H1) ? w2[j * H1 + i] : 0.0f;
    w2p[t] = v;
    w2t[(size_t)i * H2p + j] = v;
  }
}

template <int OP, bool VALUE, bool BWD>
__global__ __launch_bounds__(REX_PPO_THREADS) void rex_ppo_tile_kernel(PpoArgs p) {
  extern __shared__ __attribute__((aligned(16))) float ppo_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r32 = lane & 31, hh = lane >> 5;
  const int O = p.O, A = p.A, H1 = p.H1, H2 = p.H2, H1p = p.H1p, H2p = p.H2p, T = p.T, NT = p.NT;
  const int LD1 = H1p + 4, LD2 = H2p + 4;       // row strides = 4 (mod 32) floats: 16-byte reads of 8 consecutive rows cover the banks once
  float* xs = ppo_lds;                           // [64][OP]
  float* h1s = xs + REX_PPO_TILE * OP;           // [64][LD1]: h1, then dh1
  float* h2s = h1s + REX_PPO_TILE * LD1;         // [64][LD2]: h2, then dh2
  float* w3s = h2s + REX_PPO_TILE * LD2;         // [8][H2p]
  float* zs = w3s + REX_PPO_MAX_A * H2p;         // [8][64]
  float* gzs = zs + REX_PPO_MAX_A * REX_PPO_TILE;   // [64][8]
  float* gls = gzs + REX_PPO_MAX_A * REX_PPO_TILE;  // [16][64]: every sample lane's running sums of g_z and g_l (-> db3, d logstd)
  const float4* xs4 = reinterpret_cast<const float4*>(xs);

  // ---- what a thread keeps over all its tiles ----
  const int ju = tid & 127, half = tid >> 7;     // unit ju of layer 2, samples 32 half .. of a tile (step 6)
  const float b2r = (wave * 32 + r32 < H2) ? p.b2[wave * 32 + r32] : 0.0f;
  float dw1[OP], db1 = 0.0f, dw3[REX_PPO_MAX_A], db2 = 0.0f;
  ppo_f16 acc2[2][4];                            // dW2 tiles [input units 32 (wave + 4 nt)][output units 32 mt]
#pragma unroll
  for (int o = 0; o < OP; ++o) dw1[o] = 0.0f;
#pragma unroll
  for (int a = 0; a < REX_PPO_MAX_A; ++a) dw3[a] = 0.0f;
  for (int k = tid; k < 2 * REX_PPO_MAX_A * REX_PPO_TILE; k += REX_PPO_THREADS) gls[k] = 0.0f;
#pragma unroll
  for (int nt = 0; nt < 2; ++nt)
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc2[nt][mt][e] = 0.0f;
  for (int k = tid; k < REX_PPO_MAX_A * H2p; k += REX_PPO_THREADS) {
    const int a = k / H2p, j = k - a * H2p;
    w3s[k] = (a < A && j < H2) ? p.w3[a * H2 + j] : 0.0f;
  }

  const int tiles = p.R * NT;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int r = tile / NT, t0 = (tile - r * NT) * REX_PPO_TILE;
    const int len = ppo_row_len(p.length, r, T);
    if (t0 >= len) continue;                     // (the same for every thread of the workgroup)
    const int nvalid = min(REX_PPO_TILE, len - t0);
    const size_t base = (size_t)r * T + t0;
    __syncthreads();                             // the previous tile's last reads of xs / h1s; w3s
    // ---- 1: the observations ----
    for (int k = tid; k < REX_PPO_TILE * OP; k += REX_PPO_THREADS) {
      const int s = k / OP, o = k - s * OP;
      xs[k] = (s < nvalid && o < O) ? p.observ[(base + s) * O + o] : 0.0f;
    }
    __syncthreads();
    // ---- 2: h1 ----
    if (tid < H1p) {
      float w1r[OP];                               // unit tid's row of W1 (L2; not kept over the tile: the registers are the backward pass's)
#pragma unroll
      for (int o = 0; o < OP; ++o) w1r[o] = (tid < H1 && o < O) ? p.w1[tid * O + o] : 0.0f;
      const float b1r = tid < H1 ? p.b1[tid] : 0.0f;
#pragma clang loop unroll(disable)
      for (int s = 0; s < REX_PPO_TILE; ++s) {
        float acc = b1r;
#pragma unroll
        for (int q = 0; q < OP / 4; ++q) {
          const float4 x = xs4[s * (OP / 4) + q];
          acc = fmaf(w1r[4 * q], x.x, acc); acc = fmaf(w1r[4 * q + 1], x.y, acc); acc = fmaf(w1r[4 * q + 2], x.z, acc); acc = fmaf(w1r[4 * q + 3], x.w, acc);
        }
        h1s[s * LD1 + tid] = fmaxf(acc, 0.0f);
      }
    }
    __syncthreads();
    // ---- 3: h2 = relu(W2 h1 + b2), D[sample][unit]: A = h1 (LDS), B = W2 (L2, a ring of four reads) ----
    if (wave * 32 < H2p) {
      ppo_f16 acc[2];
#pragma unroll
      for (int e = 0; e < 16; ++e) { acc[0][e] = b2r; acc[1][e] = b2r; }
      const float4* bw = reinterpret_cast<const float4*>(p.w2p + (size_t)(wave * 32 + r32) * H1p + 4 * hh);
      const float4* a0 = reinterpret_cast<const float4*>(h1s + r32 * LD1 + 4 * hh);
      const float4* a1 = reinterpret_cast<const float4*>(h1s + (32 + r32) * LD1 + 4 * hh);
      const int n = H1p / 8;                     // groups of 8 k; a multiple of 4
      float4 ring[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) ring[u] = bw[2 * u];
#pragma clang loop unroll(disable)
      for (int g0 = 0; g0 < n; g0 += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int g = g0 + u;
          const float4 b = ring[u];
          ring[u] = bw[2 * min(g + 4, n - 1)];
          const float4 x0 = a0[2 * g], x1 = a1[2 * g];
          ppo_mfma_k4(acc[0], acc[1], x0, x1, b);
        }
      }
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int e = 0; e < 16; ++e) h2s[(32 * mt + ppo_acc_row(e, hh)) * LD2 + wave * 32 + r32] = fmaxf(acc[mt][e], 0.0f);
    }
    __syncthreads();
    // ---- 4: z = W3 h2 + b3: thread (sample tid & 63, outputs tid >> 6 and + 4) ----
    {
      const int s = tid & 63;
      const float4* h4 = reinterpret_cast<const float4*>(h2s + s * LD2);
#pragma unroll
      for (int ga = 0; ga < 2; ++ga) {
        const int a = (tid >> 6) + 4 * ga;
        if (a < A) {
          const float4* w4 = reinterpret_cast<const float4*>(w3s + a * H2p);
          float acc = p.b3[a];
#pragma clang loop unroll(disable)
          for (int q = 0; q < H2p / 4; ++q) {
            const float4 h = h4[q], w = w4[q];
            acc = fmaf(h.x, w.x, acc); acc = fmaf(h.y, w.y, acc); acc = fmaf(h.z, w.z, acc); acc = fmaf(h.w, w.w, acc);
          }
          zs[a * REX_PPO_TILE + s] = acc;
        }
      }
    }
    __syncthreads();
    // ---- 5: the loss terms and the seeds: wave 0, lane = sample ----
    if (wave == 0) {
      const int s = lane;
      const bool valid = s < nvalid;
      float gz[REX_PPO_MAX_A];
#pragma unroll
      for (int a = 0; a < REX_PPO_MAX_A; ++a) gz[a] = 0.0f;
      if constexpr (VALUE) {
        const float v = zs[s];
        const float d = valid ? p.target[base + s] - v : 0.0f;
        if (p.value_out && t0 + s < T) p.value_out[base + s] = valid ? v : 0.0f;
        const float sum = ppo_wave_sum(0.5f * d * d);
        if (lane == 0) p.part[tile] = sum;
        gz[0] = -d * p.inv_rt;
      } else {
        PpoGauss h;
        float z[REX_PPO_MAX_A];
#pragma unroll
        for (int a = 0; a < REX_PPO_MAX_A; ++a) z[a] = (a < A && valid) ? zs[a * REX_PPO_TILE + s] : 0.0f;
        ppo_gauss_terms(h, z, A, valid, p.logstd, p.old_logstd, p.old_mean, p.action, (base + s) * A);
        const float kl = h.kl, ratio = h.ratio;
        const float adv = valid ? p.target[base + s] : 0.0f;
        if constexpr (!BWD) {
          const float ksum = ppo_wave_sum(valid ? kl : 0.0f), ssum = ppo_wave_sum(valid ? ratio * adv : 0.0f);
          if (lane == 0) { p.part[tile] = ksum; p.part[tiles + tile] = ssum; }
        } else {
          const float wr = ppo_row_weight(p.kl_row[r], p.penalty, p.cutoff, p.coef);
          const float ra = ratio * adv;
#pragma unroll
          for (int a = 0; a < REX_PPO_MAX_A; ++a) {
            if (a < A && valid) {
              float gl;
              ppo_gauss_seed(h, a, wr, ra, p.inv_rt, &gz[a], &gl);
              gls[(REX_PPO_MAX_A + a) * REX_PPO_TILE + s] += gl;
            }
          }
        }
      }
      if constexpr (BWD) {
#pragma unroll
        for (int a = 0; a < REX_PPO_MAX_A; ++a) if (a < A) gls[a * REX_PPO_TILE + s] += gz[a];
        float4* g4 = reinterpret_cast<float4*>(gzs + s * REX_PPO_MAX_A);
        g4[0] = make_float4(gz[0], gz[1], gz[2], gz[3]);
        g4[1] = make_float4(gz[4], gz[5], gz[6], gz[7]);
      }
    }
    if constexpr (BWD) {
      __syncthreads();
      // ---- 6: dh2 over h2, dW3, db2: thread (unit ju, samples 32 half ..) ----
      if (ju < H2p) {
        float w3c[REX_PPO_MAX_A];
#pragma unroll
        for (int a = 0; a < REX_PPO_MAX_A; ++a) w3c[a] = w3s[a * H2p + ju];
#pragma clang loop unroll(disable)
        for (int s = 32 * half; s < 32 * half + 32; ++s) {
          const float4 ga = reinterpret_cast<const float4*>(gzs)[2 * s], gb = reinterpret_cast<const float4*>(gzs)[2 * s + 1];
          const float g[REX_PPO_MAX_A] = {ga.x, ga.y, ga.z, ga.w, gb.x, gb.y, gb.z, gb.w};
          const float h = h2s[s * LD2 + ju];
          float d = 0.0f;
#pragma unroll
          for (int a = 0; a < REX_PPO_MAX_A; ++a) { dw3[a] = fmaf(g[a], h, dw3[a]); d = fmaf(w3c[a], g[a], d); }
          d = h > 0.0f ? d : 0.0f;
          db2 += d;
          h2s[s * LD2 + ju] = d;
        }
      }
      __syncthreads();
      // ---- 7: dW2 += dh2^T h1, D[output unit][input unit], K = the samples ----
#pragma clang loop unroll(disable)
      for (int t = 0; t < REX_PPO_TILE / 2; ++t) {
        const int s = 2 * t + hh;
        float a[4], b[2];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) a[mt] = (32 * mt < H2p) ? h2s[s * LD2 + 32 * mt + r32] : 0.0f;
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) b[nt] = (32 * (wave + 4 * nt) < H1p) ? h1s[s * LD1 + 32 * (wave + 4 * nt) + r32] : 0.0f;
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
          if (32 * (wave + 4 * nt) < H1p) {
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
              if (32 * mt < H2p) acc2[nt][mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mt], b[nt], acc2[nt][mt], 0, 0, 0);
          }
      }
      __syncthreads();
      // ---- 8: dh1 = dh2 W2 . relu' over h1, D[sample][input unit], K = H2 ----
      {
        ppo_f16 acc[2][2];                       // [nt][mt]
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
          for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[nt][mt][e] = 0.0f;
        const bool on1 = 32 * (wave + 4) < H1p, on0 = 32 * wave < H1p;
        // (a wave without a second tile reads its first one's rows again: in bounds, not used)
        const float4* bw0 = reinterpret_cast<const float4*>(p.w2t + (size_t)(32 * (on0 ? wave : 0) + r32) * H2p + 4 * hh);
        const float4* bw1 = reinterpret_cast<const float4*>(p.w2t + (size_t)(32 * (on1 ? wave + 4 : 0) + r32) * H2p + 4 * hh);
        const float4* a0 = reinterpret_cast<const float4*>(h2s + r32 * LD2 + 4 * hh);
        const float4* a1 = reinterpret_cast<const float4*>(h2s + (32 + r32) * LD2 + 4 * hh);
        const int n = H2p / 8;                   // a multiple of 4
        float4 ring0[4], ring1[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { ring0[u] = bw0[2 * u]; ring1[u] = bw1[2 * u]; }
        if (on0) {
#pragma clang loop unroll(disable)
          for (int g0 = 0; g0 < n; g0 += 4) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const int g = g0 + u, gn = min(g + 4, n - 1);
              const float4 b0 = ring0[u], b1 = ring1[u];
              ring0[u] = bw0[2 * gn]; ring1[u] = bw1[2 * gn];
              const float4 x0 = a0[2 * g], x1 = a1[2 * g];
              ppo_mfma_k4(acc[0][0], acc[0][1], x0, x1, b0);
              if (on1) {
                ppo_mfma_k4(acc[1][0], acc[1][1], x0, x1, b1);
              }
            }
          }
#pragma unroll
          for (int nt = 0; nt < 2; ++nt)
            if (nt == 0 || on1) {
#pragma unroll
              for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                  const int at = (32 * mt + ppo_acc_row(e, hh)) * LD1 + 32 * (wave + 4 * nt) + r32;
                  h1s[at] = h1s[at] > 0.0f ? acc[nt][mt][e] : 0.0f;
                }
            }
        }
      }
      __syncthreads();
      // ---- 9: dW1, db1 ----
      if (tid < H1p) {
#pragma clang loop unroll(disable)
        for (int s = 0; s < REX_PPO_TILE; ++s) {
          const float d = h1s[s * LD1 + tid];
          db1 += d;
#pragma unroll
          for (int q = 0; q < OP / 4; ++q) {
            const float4 x = xs4[s * (OP / 4) + q];
            dw1[4 * q] = fmaf(d, x.x, dw1[4 * q]); dw1[4 * q + 1] = fmaf(d, x.y, dw1[4 * q + 1]);
            dw1[4 * q + 2] = fmaf(d, x.z, dw1[4 * q + 2]); dw1[4 * q + 3] = fmaf(d, x.w, dw1[4 * q + 3]);
          }
        }
      }
    }
  }

  if constexpr (BWD) {
    // ---- the workgroup's partial gradients, once ----
    const PpoOff o = ppo_offsets(O, A, H1, H2);
    float* pg = p.pgrad + (size_t)blockIdx.x * o.total;
    if (tid < H1) {
#pragma unroll
      for (int k = 0; k < OP; ++k) if (k < O) pg[o.w1 + tid * O + k] = dw1[k];
      pg[o.b1 + tid] = db1;
    }
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int j = 32 * mt + ppo_acc_row(e, hh), i = 32 * (wave + 4 * nt) + r32;
          if (j < H2 && i < H1) pg[o.w2 + j * H1 + i] = acc2[nt][mt][e];
        }
    // the two half tiles' sums of a layer-2 unit: half 0 + half 1
    __syncthreads();
    float* sw = h1s;                               // [9][128]
    if (half == 1) {
#pragma unroll
      for (int a = 0; a < REX_PPO_MAX_A; ++a) sw[a * 128 + ju] = dw3[a];
      sw[REX_PPO_MAX_A * 128 + ju] = db2;
    }
    __syncthreads();
    if (half == 0 && ju < H2) {
#pragma unroll
      for (int a = 0; a < REX_PPO_MAX_A; ++a) if (a < A) pg[o.w3 + a * H2 + ju] = dw3[a] + sw[a * 128 + ju];
      pg[o.b2 + ju] = db2 + sw[REX_PPO_MAX_A * 128 + ju];
    }
    if (wave == 0) {
#pragma unroll
      for (int a = 0; a < REX_PPO_MAX_A; ++a) {
        const float gs = ppo_wave_sum(gls[a * REX_PPO_TILE + lane]), ls = ppo_wave_sum(gls[(REX_PPO_MAX_A + a) * REX_PPO_TILE + lane]);
        if (lane == 0 && a < A) { pg[o.b3 + a] = gs; pg[o.logstd + a] = ls; }
      }
    }
  }
}

// the per-tile sums -> kl_row [R] and the scalar loss, in a fixed order: one workgroup, a thread adds its rows' tiles, then a tree
template <bool VALUE>
__global__ __launch_bounds__(REX_PPO_THREADS) void rex_ppo_rows_kernel(PpoArgs p, float* __restrict__ loss, float* __restrict__ kl_row) {
  const int tid = threadIdx.x, tiles = p.R * p.NT;
  float acc = 0.0f;
  for (int r = tid; r < p.R; r += REX_PPO_THREADS) {
    const int len = ppo_row_len(p.length, r, p.T), nt = (len + REX_PPO_TILE - 1) / REX_PPO_TILE;
    float a = 0.0f, b = 0.0f;
    for (int k = 0; k < nt; ++k) { a += p.part[r * p.NT + k]; if (!VALUE) b += p.part[tiles + r * p.NT + k]; }
    if (VALUE) acc += a;
    else {
      float kl;
      const float term = ppo_row_loss(a, b, p.T, p.penalty, p.cutoff, p.coef, &kl);
      kl_row[r] = kl;
      acc += term;
    }
  }
  const float* red = ppo_block_sum(tid, acc);
  if (tid == 0) *loss = VALUE ? red[0] / ((float)p.R * (float)p.T) : red[0] / (float)p.R;
}

// grad = the workgroups' partials added in index order; the seven tensors are the caller's (torch layout)
struct PpoGradDev { float *w1, *b1, *w2, *b2, *w3, *b3, *logstd; };
__global__ __launch_bounds__(256) void rex_ppo_reduce_kernel(const float* __restrict__ pgrad, int groups, PpoOff o, int nparams, PpoGradDev g) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nparams) return;
  float acc = 0.0f;
  for (int b = 0; b < groups; ++b) acc += pgrad[(size_t)b * o.total + k];
  if (k < o.b1) g.w1[k] = acc;
  else if (k < o.w2) g.b1[k - o.b1] = acc;
  else if (k < o.b2) g.w2[k - o.w2] = acc;
  else if (k < o.w3) g.b2[k - o.b2] = acc;
  else if (k < o.b3) g.w3[k - o.w3] = acc;
  else if (k < o.logstd) g.b3[k - o.b3] = acc;
  else g.logstd[k - o.logstd] = acc;
}

// one lane per episode row, a reverse scan: utility.py:71-81 (discounted_return) and, with a value block, utility.py:97-110 (lambda_return).
// The products and sums are separate statements: two roundings each, as the reference's tensor operations have.
__global__ __launch_bounds__(64) void rex_ppo_returns_kernel(int R, int T, const float* __restrict__ reward, const int32_t* __restrict__ length, float discount,
                                                            float* __restrict__ ret, const float* __restrict__ value, float lambda, float one_minus_lambda,
                                                            float* __restrict__ lret) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const int len = length[r];
  const size_t row = (size_t)r * T;
  float agg = 0.0f, lagg = 0.0f;
  for (int t = T - 1; t >= 0; --t) {
    const bool in = t < len;
    const float rew = in ? reward[row + t] : 0.0f;
    if (ret) {
      const float d = discount * agg;
      agg = rew + d;
      ret[row + t] = agg;
    }
    if (lret) {
      const float dv = discount * value[row + t];
      const float boot = dv * one_minus_lambda;
      const float seq = rew + boot;
      const float dl = in ? discount * lambda : 0.0f;
      const float carried = dl * lagg;
      lagg = seq + carried;
      lret[row + t] = lagg;
    }
  }
}

typedef void (*PpoTileKernel)(PpoArgs);
template <bool VALUE, bool BWD> static PpoTileKernel ppo_tile_kernel(int OP) {
  return OP == 4 ? &rex_ppo_tile_kernel<4, VALUE, BWD> : OP == 16 ? &rex_ppo_tile_kernel<16, VALUE, BWD> : &rex_ppo_tile_kernel<24, VALUE, BWD>;
}

}  // namespace rex

// rex_learner.hip -- the C ABI (include/rexsim.h) of the fused PPO learners: the shape and pointer checks, the workspace layout and the
// launch sequences of the kernels of rex_learner.h (forward policy, value net, return scans) and rex_learner_rnn.h (recurrent policy).
#include "rex_error.h"
#include "rex_learner.h"
#include "rex_learner_rnn.h"
#include <algorithm>
#include <cstdio>
#include <vector>

#define PPO_LAUNCH(...)                \
  do {                                 \
    hipLaunchKernelGGL(__VA_ARGS__);   \
    HIPCHK(hipGetLastError());         \
  } while (0)

// ---- what both learners check ----
// hidden_error: what the caller found wrong with the network's own widths (nullptr: nothing), reported in its place between out_dim and
// the memory's shape
static int ppo_check_dims(const char* who, int rows, int steps, int obs_dim, int out_dim, bool value, const char* hidden_error) {
  if (obs_dim != 4 && obs_dim != 16 && obs_dim != 22) return failf(REX_EINVAL, "%s: obs_dim %d is not offered (4, 16 or 22)", who, obs_dim);
  if (value ? out_dim != 1 : (out_dim != 1 && out_dim != 2 && out_dim != 4 && out_dim != 8))
    return failf(REX_EINVAL, "%s: out_dim %d is not offered (%s)", who, out_dim, value ? "the value net has one output" : "action_dim 1, 2, 4 or 8");
  if (hidden_error) return failf(REX_EINVAL, "%s: %s", who, hidden_error);
  if (rows < 1 || steps < 1 || (long long)rows * steps * 24 >= (1ll << 31))
    return failf(REX_EINVAL, "%s: a memory of %d rows x %d steps is not offered (rows, steps >= 1, rows * steps * 24 < 2^31)", who, rows, steps);
  return REX_OK;
}
static int ppo_check_batch(const char* who, const RexPpoBatch* b, bool value) {
  if (!b->d_observ || !b->d_length || (value ? !b->d_return : (!b->d_action || !b->d_old_mean || !b->d_old_logstd || !b->d_advantage)))
    return failf(REX_EINVAL, "%s: null memory block", who);
  return REX_OK;
}
// more than 64 KB of dynamic LDS needs the function's limit raised: once per (kernel, device) and size, not per launch
static hipError_t raise_lds_limit(const void* f, size_t lds) {
  struct Raised { const void* f; int device; size_t bytes; };
  static thread_local std::vector<Raised> raised;
  int device = 0;
  hipError_t e = hipGetDevice(&device);
  if (e != hipSuccess) return e;
  auto it = std::find_if(raised.begin(), raised.end(), [&](const Raised& r) { return r.f == f && r.device == device; });
  if (it == raised.end() || it->bytes < lds) {
    e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    if (it == raised.end()) raised.push_back({f, device, lds}); else it->bytes = lds;
  }
  return hipSuccess;
}
template <class Args>
static hipError_t launch_lds(void (*k)(Args), int groups, int threads, size_t lds, hipStream_t st, const Args& a) {
  const hipError_t e = raise_lds_limit(reinterpret_cast<const void*>(k), lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k, dim3(groups), dim3(threads), lds, st, a);
  return hipGetLastError();
}

// ---- the forward learner (rex_learner.h) ----
static int ppo_check_shape(const char* who, int rows, int steps, int O, int A, int H1, int H2, bool value) {
  char bad[128] = "";
  if (H1 < 1 || H1 > REX_PPO_MAX_H1 || H2 < 1 || H2 > REX_PPO_MAX_H2)
    snprintf(bad, sizeof(bad), "hidden layers of %d and %d units are not offered (1..%d and 1..%d)", H1, H2, REX_PPO_MAX_H1, REX_PPO_MAX_H2);
  return ppo_check_dims(who, rows, steps, O, A, value, bad[0] ? bad : nullptr);
}

static int ppo_loss(const char* who, bool value, const RexPpoNet* net, const RexPpoBatch* b, const RexPpoGrad* grad, float* d_loss, float* d_kl_row, float* d_value_out,
                    void* d_workspace, hipStream_t st) {
  if (!net || !b) return failf(REX_EINVAL, "%s: null pointer", who);
  const int O = net->obs_dim, A = net->out_dim, H1 = net->hidden1, H2 = net->hidden2, R = b->rows, T = b->steps;
  int rc = ppo_check_shape(who, R, T, O, A, H1, H2, value);
  if (rc != REX_OK) return rc;
  if (!net->d_w1 || !net->d_b1 || !net->d_w2 || !net->d_b2 || !net->d_w3 || !net->d_b3 || (!value && !net->d_logstd)) return failf(REX_EINVAL, "%s: null weight pointer", who);
  if ((rc = ppo_check_batch(who, b, value)) != REX_OK) return rc;
  if (!d_loss || !d_workspace || (!value && !d_kl_row)) return failf(REX_EINVAL, "%s: null output or workspace pointer", who);
  if (grad && (!grad->d_w1 || !grad->d_b1 || !grad->d_w2 || !grad->d_b2 || !grad->d_w3 || !grad->d_b3 || (!value && !grad->d_logstd)))
    return failf(REX_EINVAL, "%s: null gradient pointer (pass grad = NULL for a forward-only call)", who);
  const rex::PpoWs ws = rex::ppo_workspace(R, T, O, A, H1, H2);
  float* w = static_cast<float*>(d_workspace);
  rex::PpoArgs a{};
  a.w1 = net->d_w1; a.b1 = net->d_b1; a.b2 = net->d_b2; a.w3 = net->d_w3; a.b3 = net->d_b3; a.logstd = net->d_logstd;
  a.w2p = w + ws.w2p; a.w2t = w + ws.w2t; a.part = w + ws.part; a.pgrad = w + ws.pgrad;
  a.observ = b->d_observ; a.action = b->d_action; a.old_mean = b->d_old_mean; a.old_logstd = b->d_old_logstd;
  a.target = value ? b->d_return : b->d_advantage;
  a.length = b->d_length; a.kl_row = d_kl_row; a.value_out = d_value_out;
  a.O = O; a.A = A; a.H1 = H1; a.H2 = H2; a.H1p = rex::ppo_up(H1, 32); a.H2p = rex::ppo_up(H2, 32); a.R = R; a.T = T; a.NT = ws.ntiles;
  a.penalty = b->penalty; a.cutoff = b->kl_cutoff; a.coef = b->kl_cutoff_coef;
  a.inv_rt = (float)(1.0 / ((double)R * (double)T));
  const int OP = O == 22 ? 24 : O;
  const size_t lds = sizeof(float) * (size_t)rex::ppo_lds_floats(OP, a.H1p, a.H2p);
  auto launch = [&](rex::PpoTileKernel k) { return launch_lds(k, ws.groups, REX_PPO_THREADS, lds, st, a); };
  PPO_LAUNCH(rex::rex_ppo_pack_kernel, dim3((a.H1p * a.H2p + 255) / 256), dim3(256), 0, st, net->d_w2, H1, H2, a.H1p, a.H2p, w + ws.w2p, w + ws.w2t);
  if (value) {
    // one pass: the tiles' loss terms come out of the same pass as the gradients (tiles beyond a row's length are skipped: their values are zero)
    if (d_value_out) HIPCHK(hipMemsetAsync(d_value_out, 0, sizeof(float) * (size_t)R * T, st));
    HIPCHK(launch(grad ? rex::ppo_tile_kernel<true, true>(OP) : rex::ppo_tile_kernel<true, false>(OP)));
    PPO_LAUNCH(rex::rex_ppo_rows_kernel<true>, dim3(1), dim3(REX_PPO_THREADS), 0, st, a, d_loss, (float*)nullptr);
  } else {
    // two phases: w_r of the seeds needs the whole row's KL -- forward only (loss, kl_row), then forward + backward
    HIPCHK(launch(rex::ppo_tile_kernel<false, false>(OP)));
    PPO_LAUNCH(rex::rex_ppo_rows_kernel<false>, dim3(1), dim3(REX_PPO_THREADS), 0, st, a, d_loss, d_kl_row);
    if (grad) HIPCHK(launch(rex::ppo_tile_kernel<false, true>(OP)));
  }
  if (grad) {
    const rex::PpoOff o = rex::ppo_offsets(O, A, H1, H2);
    const int np = value ? o.logstd : o.logstd + A;
    const rex::PpoGradDev g{grad->d_w1, grad->d_b1, grad->d_w2, grad->d_b2, grad->d_w3, grad->d_b3, grad->d_logstd};
    PPO_LAUNCH(rex::rex_ppo_reduce_kernel, dim3((np + 255) / 256), dim3(256), 0, st, (const float*)(w + ws.pgrad), ws.groups, o, np, g);
  }
  return REX_OK;
}

// ---- the recurrent learner (rex_learner_rnn.h) ----
static int rnn_check_shape(const char* who, int rows, int steps, int obs_dim, int out_dim, int hidden1, int state) {
  if (state != REX_RNN_H) return failf(REX_EINVAL, "%s: state %d is not offered (the GRU cell has %d units)", who, state, REX_RNN_H);
  char bad[128] = "";
  if (hidden1 < 1 || hidden1 > REX_PPO_MAX_H1) snprintf(bad, sizeof(bad), "hidden1 %d is not offered (1..%d)", hidden1, REX_PPO_MAX_H1);
  return ppo_check_dims(who, rows, steps, obs_dim, out_dim, false, bad[0] ? bad : nullptr);
}

extern "C" {

long long rex_ppo_workspace_bytes(int rows, int steps, int obs_dim, int out_dim, int hidden1, int hidden2) {
  if (ppo_check_shape("rex_ppo_workspace_bytes", rows, steps, obs_dim, out_dim, hidden1, hidden2, false) != REX_OK) return REX_EINVAL;
  return (long long)(sizeof(float) * rex::ppo_workspace(rows, steps, obs_dim, out_dim, hidden1, hidden2).total);
}

int rex_ppo_returns(int rows, int steps, const float* d_reward, const int32_t* d_length, float discount, float* d_return, const float* d_value, float lambda,
                    float* d_lambda_return, void* stream) {
  if (rows < 1 || steps < 1 || (long long)rows * steps >= (1ll << 31) || !d_reward || !d_length || (!d_return && !d_lambda_return) || (d_lambda_return && !d_value))
    return fail(REX_EINVAL, "rex_ppo_returns: bad arguments (rows, steps >= 1, rows * steps < 2^31, an output, d_value with d_lambda_return)%s", "");
  PPO_LAUNCH(rex::rex_ppo_returns_kernel, dim3((rows + 63) / 64), dim3(64), 0, (hipStream_t)stream, rows, steps, d_reward, d_length, discount, d_return, d_value,
             lambda, (float)(1.0 - (double)lambda), d_lambda_return);
  return REX_OK;
}

int rex_ppo_policy_loss(const RexPpoNet* net, const RexPpoBatch* batch, const RexPpoGrad* grad, float* d_loss, float* d_kl_row, void* d_workspace, void* stream) {
  return ppo_loss("rex_ppo_policy_loss", false, net, batch, grad, d_loss, d_kl_row, nullptr, d_workspace, (hipStream_t)stream);
}

int rex_ppo_value_loss(const RexPpoNet* net, const RexPpoBatch* batch, const RexPpoGrad* grad, float* d_loss, float* d_value_out, void* d_workspace, void* stream) {
  return ppo_loss("rex_ppo_value_loss", true, net, batch, grad, d_loss, nullptr, d_value_out, d_workspace, (hipStream_t)stream);
}

long long rex_ppo_recurrent_workspace_bytes(int rows, int steps, int obs_dim, int out_dim, int hidden1, int state) {
  if (rnn_check_shape("rex_ppo_recurrent_workspace_bytes", rows, steps, obs_dim, out_dim, hidden1, state) != REX_OK) return REX_EINVAL;
  return (long long)(sizeof(float) * rex::rnn_workspace(rows, steps, obs_dim, hidden1).total);
}

int rex_ppo_recurrent_policy_loss(const RexPpoRnnNet* net, const RexPpoBatch* b, const RexPpoRnnGrad* grad, float* d_loss, float* d_kl_row, void* d_workspace,
                                  void* stream) {
  const char* who = "rex_ppo_recurrent_policy_loss";
  if (!net || !b) return failf(REX_EINVAL, "%s: null pointer", who);
  int rc = rnn_check_shape(who, b->rows, b->steps, net->obs_dim, net->out_dim, net->hidden1, net->state);
  if (rc != REX_OK) return rc;
  if (!net->d_w1 || !net->d_b1 || !net->d_wg || !net->d_bg || !net->d_wc || !net->d_bc || !net->d_wm || !net->d_bm || !net->d_logstd)
    return failf(REX_EINVAL, "%s: null weight pointer", who);
  if ((rc = ppo_check_batch(who, b, false)) != REX_OK) return rc;
  if (!d_loss || !d_kl_row || !d_workspace) return failf(REX_EINVAL, "%s: null output or workspace pointer", who);
  if (grad && (!grad->d_w1 || !grad->d_b1 || !grad->d_wg || !grad->d_bg || !grad->d_wc || !grad->d_bc || !grad->d_wm || !grad->d_bm || !grad->d_logstd))
    return failf(REX_EINVAL, "%s: null gradient pointer (pass grad = NULL for a forward-only call)", who);
  hipStream_t st = (hipStream_t)stream;
  const int O = net->obs_dim, A = net->out_dim, F = net->hidden1, R = b->rows, T = b->steps, H = REX_RNN_H;
  const rex::RnnWs ws = rex::rnn_workspace(R, T, O, F);
  float* w = static_cast<float*>(d_workspace);
  rex::RnnArgs a{};
  a.w1 = net->d_w1; a.b1 = net->d_b1; a.wg = net->d_wg; a.bg = net->d_bg; a.wc = net->d_wc; a.bc = net->d_bc; a.wm = net->d_wm; a.bm = net->d_bm; a.logstd = net->d_logstd;
  a.observ = b->d_observ; a.action = b->d_action; a.old_mean = b->d_old_mean; a.old_logstd = b->d_old_logstd; a.advantage = b->d_advantage; a.length = b->d_length;
  a.wht = w + ws.wht; a.wh = w + ws.wh; a.wxp = w + ws.wxp; a.wxt = w + ws.wxt; a.biasp = w + ws.biasp; a.x = w + ws.x; a.act = w + ws.act; a.hs = w + ws.hs;
  a.rh = w + ws.rh; a.gzl = w + ws.gzl; a.klt = w + ws.klt; a.sat = w + ws.sat; a.rowloss = w + ws.rowloss; a.pw = w + ws.pw; a.pb = w + ws.pb; a.pm = w + ws.pm;
  a.pz = w + ws.pz; a.p1 = w + ws.p1; a.kl_row = d_kl_row;
  a.O = O; a.A = A; a.F = F; a.Fp = ws.Fp; a.R = R; a.T = T; a.NT = ws.ntiles; a.ksplit = ws.ksplit; a.osplit = ws.osplit;
  a.penalty = b->penalty; a.cutoff = b->kl_cutoff; a.coef = b->kl_cutoff_coef;
  a.inv_rt = (float)(1.0 / ((double)R * (double)T));
  const size_t N = (size_t)R * T;
  const int tiles = R * ws.ntiles, scan_groups = (R + REX_RNN_ROWS - 1) / REX_RNN_ROWS;
  const size_t lds = sizeof(float) * (size_t)rex::rnn_scan_lds_floats();
  const unsigned slots = (unsigned)((N + 255) / 256);
  PPO_LAUNCH(rex::rex_rnn_pack_kernel, dim3((std::max(REX_RNN_GP * ws.Fp, 3 * H * H) + 255) / 256), dim3(256), 0, st, a);
  PPO_LAUNCH(rex::rex_rnn_input_kernel, dim3((unsigned)((N * ws.Fp + 255) / 256)), dim3(256), 0, st, a);
  PPO_LAUNCH(rex::rex_rnn_rows_kernel<false>, dim3(tiles), dim3(256), 0, st, a);
  HIPCHK(launch_lds(&rex::rex_rnn_scan_fwd_kernel, scan_groups, REX_RNN_SCAN_THREADS, lds, st, a));
  PPO_LAUNCH(rex::rex_rnn_head_kernel<false>, dim3(slots), dim3(256), 0, st, a);
  PPO_LAUNCH(rex::rex_rnn_rowsum_kernel, dim3(R), dim3(REX_PPO_THREADS), 0, st, a, d_kl_row);
  PPO_LAUNCH(rex::rex_rnn_loss_kernel, dim3(1), dim3(REX_PPO_THREADS), 0, st, a, d_loss);
  if (!grad) return REX_OK;
  PPO_LAUNCH(rex::rex_rnn_head_kernel<true>, dim3(slots), dim3(256), 0, st, a);
  HIPCHK(launch_lds(&rex::rex_rnn_scan_bwd_kernel, scan_groups, REX_RNN_SCAN_THREADS, lds, st, a));
  const int NI = (ws.Fp + REX_RNN_HP) / 32;
  PPO_LAUNCH(rex::rex_rnn_wgrad_kernel, dim3((6 * NI + 3) / 4, ws.ksplit), dim3(256), 0, st, a);
  PPO_LAUNCH(rex::rex_rnn_outer_kernel<0>, dim3(REX_RNN_GP / 128, ws.osplit), dim3(128), 0, st, a, (const float*)nullptr, 0, (const float*)a.act, REX_RNN_GP, REX_RNN_GP, a.pb);
  PPO_LAUNCH(rex::rex_rnn_outer_kernel<8>, dim3(1, ws.osplit), dim3(128), 0, st, a, (const float*)a.gzl, 16, (const float*)a.hs, REX_RNN_HP, H, a.pm);
  PPO_LAUNCH(rex::rex_rnn_outer_kernel<0>, dim3(1, ws.osplit), dim3(128), 0, st, a, (const float*)nullptr, 0, (const float*)a.gzl, 16, 16, a.pz);
  PPO_LAUNCH(rex::rex_rnn_rows_kernel<true>, dim3(tiles), dim3(256), 0, st, a);      // X <- da1 (the weight-gradient product has read X)
  const dim3 g1((ws.Fp + 127) / 128, ws.osplit);
  if (O == 4) hipLaunchKernelGGL(rex::rex_rnn_outer_kernel<4>, g1, dim3(128), 0, st, a, a.observ, O, (const float*)a.x, ws.Fp, ws.Fp, a.p1);
  else if (O == 16) hipLaunchKernelGGL(rex::rex_rnn_outer_kernel<16>, g1, dim3(128), 0, st, a, a.observ, O, (const float*)a.x, ws.Fp, ws.Fp, a.p1);
  else hipLaunchKernelGGL(rex::rex_rnn_outer_kernel<22>, g1, dim3(128), 0, st, a, a.observ, O, (const float*)a.x, ws.Fp, ws.Fp, a.p1);
  HIPCHK(hipGetLastError());
  const int np = F * O + F + 3 * H * (F + H) + 3 * H + A * H + 2 * A;
  const rex::RnnGradDev g{grad->d_w1, grad->d_b1, grad->d_wg, grad->d_bg, grad->d_wc, grad->d_bc, grad->d_wm, grad->d_bm, grad->d_logstd};
  PPO_LAUNCH(rex::rex_rnn_final_kernel, dim3((np + 255) / 256), dim3(256), 0, st, a, g);
  return REX_OK;
}

}  // extern "C"

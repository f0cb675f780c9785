// ppo_update.hip -- the PPO update (go1_gym_learn/ppo_cse/ppo.py:98-206) as hand-written HIP for MI355X
// (gfx950).  C ABI in include/go1_ppo.h; host mirror legged_tracking_amd/rollout.py (PPO.update).
//
// One mini-batch of PPO.update is a fixed chain of launches (go1_ppo_grad / go1_ppo_step), every one of them
// stream-ordered and graph-capturable:
//
//   phase 0 (ppo.py:107-159)                                  phase 1 (ppo.py:169-198)
//   xw<F>   adaptation L1  hist(gathered) -> a1a (256)        xw<F>   adaptation L1 (new weights) -> a1a
//   xw<F>   adaptation L2  a1a -> a2a (128)                   xw<F>   adaptation L2 -> a2a
//   adapt<FWD>  adaptation L3  a2a -> latent (priv)           adapt<MSE>  L3, mse loss vs privileged_obs on the
//   xw<F>   actor L1 [hist, latent], critic L1 [hist, priv]               first 4/5 of the rows, backward to a2a
//   xw<F>   actor / critic L2, L3                             xw<D>   delta a1a
//   head    actor L4 + critic L4, log-prob, ratio, clipped    wgrad   adaptation L1, L2 weight gradients
//           surrogate, clipped value loss, KL, entropy        reduce  -> grads (adaptation slice), aux
//           gradient; backward through L4 -> delta a3         finalize, adam (adaptation optimizer), pack
//   xw<D>   delta a2 (= W3^T delta3 * ELU'), delta a1
//   adapt<BWD> d latent = W1[:, hist:]^T delta1, backward through adaptation L3 -> delta a2a
//   xw<D>   delta a1a
//   wgrad   every weight gradient of the GEMM layers (one grouped launch, split over row chunks)
//   reduce  partials -> flat gradient (+ loss / KL sums); [all-reduce at world > 1]
//   norm, finalize (KL -> learning rate, clip_grad_norm_), adam (all parameters), pack
//
// With the height-map encoder in front of the heads (go1_ppo_dims.enc_mode = GO1_PPO_ENC_MLP; ppo_cse_cnn) the
// gathered row is G = [emb (E) | s | s | latent | priv]: s the scalars of the row's last frame, emb the encoder's
// output, first so that the xw kernel writes it in place with 16-byte stores (the module's column order is
// [s | s | emb]: pack_kernel maps the first layers' weight columns, reduce's segments map their gradients back).
//   phase 0  gather<ENC> (scalars, the map into its own padded buffer); xw<F> map -> e1 (256), xw<F> e1 -> emb into
//            G; the heads as above; then xw<LIN> W_P0[:, emb]^T delta1p, W_C0[:, emb]^T delta1c, W_A0[:, emb]^T
//            delta1a, embgrad (their sum * ELU'(emb), column sums), xw<D> delta e1; the two encoder weight
//            gradients join the grouped wgrad launch.  One encoder pass serves the three heads.
//   phase 1  xw<F> x 2 again (the encoder's weights moved in step 0), the adaptation module as above, xw<D> d emb =
//            (W_A0[:, emb]^T delta1a) * ELU'(emb), xw<D> delta e1, wgrad of four layers; Adam and the re-pack
//            cover encoder + adaptation module (the adaptation optimizer's slice, with its own moments).
//
// With the CNN encoder (enc_mode = GO1_PPO_ENC_CNN, the (2, 61, 31) map; ppo_conv.h) the encoder's part of the chain is
//   phase 0  conv<fwd> map -> feat (3360) and max feat, xw<LIN> feat -> emb into G (no activation); the heads; the
//            three xw<LIN> products and embgrad without the ELU' factor (d emb, its column sums = the linear layer's
//            bias gradient), xw<LIN> d feat = d emb W over the transposed image padded to 3456 columns (max |d feat|),
//            conv<bwd> (the forward again in LDS, then the filters' gradient partials); the linear layer's weight
//            gradient joins the grouped wgrad launch, the conv partials the reduce (four segments)
//   phase 1  conv<fwd>, xw<LIN> again; d emb = W_A0[:, emb]^T delta1a (xw<LIN>, embgrad with that one source),
//            d feat, conv<bwd>; Adam and the re-pack (conv_pack + pack) cover [conv1 | conv2 | linear | adaptation]
//
// GEMMs ("xw": activations x weights^T, "wgrad": delta^T x activations) run on v_mfma_f32_16x16x32_f16 with
// f32 accuracy from the 3xF16 split (hi = f16(x), lo = f16(x - hi), products hi*hi + hi*lo + lo*hi, f32
// accumulation; the dropped lo*lo term is ~2^-22 of a product).  Every operand tensor is first scaled by an
// exact power of two that puts its largest magnitude in [2^14, 2^15): f16's range is then never left, and the
// lo halves stay normal for every element within 2^17 of the tensor's maximum (gradients of a mean over
// 24,576 samples are ~1e-5..1e-8: unscaled they would fall into f16's subnormals).  Producers record max |x|
// (one atomicMax per wave); consumers derive the scale from it; the product is unscaled in the epilogue.
// Weights are split once per optimiser step into fragment images (forward and transposed) by the pack kernel.
//
// This file is the library's one translation unit: the launch chain above (grad_phase0, grad_phase1, step_phase)
// and the C ABI.  The rest lives in headers, one per concern, included below in dependency order:
//   ppo_split.h   vector types, tile constants, the scaling and the 3xF16 split, cross-lane sums, ELU
//   ppo_xw.h      xw_kernel, its problem builder and launch          ppo_wgrad.h   wgrad_kernel, likewise
//   ppo_gather.h  gather_kernel, embgrad_kernel                      ppo_heads.h   head_kernel, adapt_kernel
//   ppo_step.h    reduce, norm, finalize, adam, wmax / pack, absmax, zero, and the tables they take
//   ppo_conv.h    conv_pack_kernel, conv_kernel: the CNN encoder's convolution stack, forward and backward
//   ppo_layout.h  host only: slots, the workspace layout, the table of the GEMM layers and the problems of a layer
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <string>

#include "../../include/go1_ppo.h"

namespace {

thread_local std::string g_err;
int fail(int code, const std::string& m) {
  g_err = m;
  return code;
}
#define PPO_TRY(x)                                                                        \
  do {                                                                                    \
    hipError_t e_ = (x);                                                                  \
    if (e_ != hipSuccess) return fail(GO1_PPO_E_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); \
  } while (0)

}  // namespace

#include "ppo_split.h"
#include "ppo_xw.h"
#include "ppo_wgrad.h"
#include "ppo_gather.h"
#include "ppo_heads.h"
#include "ppo_step.h"
#include "ppo_conv.h"
#include "ppo_layout.h"

namespace {

int check_ctx(const go1_ppo_dims* d, const go1_ppo_bufs* b, Ctx& C, void* stream) {
  std::string err;
  if (!make_layout(d, C.L, err)) return fail(GO1_PPO_E_ARG, err);
  if (!b || !b->params || !b->grads || !b->work || !b->hyper)
    return fail(GO1_PPO_E_ARG, "go1_ppo: params, grads, hyper and work are required");
  if ((((uintptr_t)b->work) & 255) != 0) return fail(GO1_PPO_E_ARG, "go1_ppo: work must be 256-byte aligned");
  C.d = d;
  C.b = b;
  C.ws = (char*)b->work;
  C.s = (hipStream_t)stream;
  return GO1_PPO_OK;
}

// ------------------------------------------------------------------ the launches of a layer, or of a pair
// adaptation_only: the adaptation optimizer's slice (with an encoder, the encoder's two layers as well)
int pack_weights(const Ctx& C, bool adaptation_only, bool zero_max) {
  const Lay& L = C.L;
  PackBuilder PB;
  for (int w = 0; w < L.nW; ++w)
    if (!adaptation_only || L.layer[w].adapt) PB.add(C.pack(w));
  if (zero_max) {  // otherwise finalize_kernel cleared them
    hipLaunchKernelGGL(zero_u32_kernel, dim3(1), dim3(64), 0, C.s, C.wmax(0), L.nW);
    PPO_TRY(hipGetLastError());
  }
  if (L.enc == GO1_PPO_ENC_CNN) {  // the conv filters' images: the encoder is in both slices
    hipLaunchKernelGGL(conv_pack_kernel, dim3(1), dim3(256), 0, C.s, C.conv_pack());
    PPO_TRY(hipGetLastError());
  }
  return launch_pack(C.s, PB);
}

int forward(const Ctx& C, int w, int w2 = -1) {
  const XwProb p = C.fwd(w), p2 = w2 >= 0 ? C.fwd(w2) : XwProb{};
  return launch_xw(C.s, C.L.M, C.L.layer[w].lin ? EPI_LIN : EPI_ELU, p, w2 >= 0 ? &p2 : nullptr);
}

int backward(const Ctx& C, int w, int w2 = -1) {
  const XwProb p = C.bwd(w), p2 = w2 >= 0 ? C.bwd(w2) : XwProb{};
  return launch_xw(C.s, C.L.M, EPI_DELU, p, w2 >= 0 ? &p2 : nullptr);
}

// the weight gradients of a phase's GEMM layers, one grouped launch
int weight_grads(const Ctx& C, int phase) {
  const Lay& L = C.L;
  const int order[W_N] = {W_P0, W_C0, W_P2, W_C2, W_P4, W_C4, W_A0, W_A2, W_E2, W_E0};
  WgProb ps[MAX_WG];
  int np = 0;
  for (int w : order)
    if (w < L.nW && (phase == 0 || L.layer[w].adapt)) ps[np++] = C.wg(w);
  return launch_wg(C.s, L.M, L.S[phase], L.chunk[phase], ps, np);
}

// the gradient segments of the adaptation optimizer's slice: [encoder], adaptation module
void adapt_slice_segments(const Ctx& C, SegBuilder& SB, int phase) {
  const Lay& L = C.L;
  if (L.enc == GO1_PPO_ENC_CNN) {
    C.conv_segs(SB);
    C.segs(SB, W_CNN, phase);
  } else if (L.enc) {
    C.segs(SB, W_E0, phase);
    C.segs(SB, W_E2, phase);
  }
  C.segs(SB, W_A0, phase);
  C.segs(SB, W_A2, phase);
  const AdaptPart o(L.P);
  const float* ap = C.at<float>(L.apart);
  SB.add(C.gW(IA4), ap + o.dW3a, 1, L.P * 128, 0, L.HB, adapt_stride(L.P));
  SB.add(C.gB(IA4), ap + o.db3a, 1, L.P, 0, L.HB, adapt_stride(L.P));
}

// ------------------------------------------------------------------ the arguments of the other kernels
GatherArgs gather_args(const Ctx& C) {
  const Lay& L = C.L;
  const go1_ppo_bufs* b = C.b;
  GatherArgs ga{};
  ga.hist = b->obs_history;
  ga.hld = b->hist_ld;
  ga.priv = b->privileged_obs;
  ga.act = b->actions;
  ga.mu = b->mu;
  ga.sigma = b->sigma;
  ga.logp = b->actions_log_prob;
  ga.adv = b->advantages;
  ga.ret = b->returns;
  ga.val = b->values;
  ga.idx = b->idx;
  ga.M = L.M;
  ga.H = L.H;
  ga.P = L.P;
  ga.A = L.A;
  ga.ldg = L.ldg;
  ga.bw = L.bw;
  ga.G = C.at<float>(L.G);
  ga.B = C.at<float>(L.Bb);
  ga.mx = C.mx(MX_G);
  if (L.enc) {
    ga.E = L.E;
    ga.S = L.SC;
    ga.foff = L.foff;
    ga.NM = L.NM;
    ga.ldm = L.ldm;
    ga.Mp = C.at<float>(L.mapb);
    ga.mxmap = C.mx(MX_MAP);
  }
  return ga;
}

AdaptArgs adapt_args(const Ctx& C) {
  const Lay& L = C.L;
  AdaptArgs AD{};
  AD.M = L.M;
  AD.P = L.P;
  AD.hist = L.H;
  AD.num_train = L.num_train;
  AD.ldg = L.ldg;
  AD.a2a = C.at<float>(L.a2a);
  AD.w3a = C.W(IA4);
  AD.b3a = C.B(IA4);
  AD.G = C.at<float>(L.G);
  AD.latmax = C.mx(MX_LAT);
  AD.d1p = C.at<float>(L.d1p);
  AD.w1p = C.W(IP0);
  AD.hyper = C.b->hyper;
  AD.d2a = C.at<float>(L.d2a);
  AD.d2amax = C.mx(MX_D2A);
  AD.part = C.at<float>(L.apart);
  AD.lstr = adapt_stride(L.P);
  return AD;
}

HeadArgs head_args(const Ctx& C) {
  const Lay& L = C.L;
  HeadArgs HD{};
  HD.M = L.M;
  HD.A = L.A;
  HD.bw = L.bw;
  HD.B = C.at<float>(L.Bb);
  HD.a3p = C.at<float>(L.p3);
  HD.a3c = C.at<float>(L.c3);
  HD.w4p = C.W(IP6);
  HD.b4p = C.B(IP6);
  HD.w4c = C.W(IC6);
  HD.b4c = C.B(IC6);
  HD.std_ = C.b->params + L.pstd;
  HD.hyper = C.b->hyper;
  HD.d3p = C.at<float>(L.d3p);
  HD.d3c = C.at<float>(L.d3c);
  HD.d3pmax = C.mx(MX_D3P);
  HD.d3cmax = C.mx(MX_D3C);
  HD.part = C.at<float>(L.hpart);
  HD.hstr = head_stride(L.A);
  return HD;
}

EmbArgs emb_args(const Ctx& C) {
  const Lay& L = C.L;
  EmbArgs ea{};
  ea.tp = C.at<float>(L.tp);
  ea.tc = C.at<float>(L.tc);
  ea.ta = C.at<float>(L.ta);
  ea.emb = C.at<float>(L.G);
  ea.lde = L.ldg;
  ea.demb = C.at<float>(L.demb);
  ea.colsum = C.at<float>(L.csemb);
  ea.dmax = C.mx(MX_DEMB);
  ea.M = L.M;
  ea.E = L.E;
  ea.act = L.enc != GO1_PPO_ENC_CNN;
  ea.nsrc = 3;
  return ea;
}

// the encoder's forward into G's leading columns: the MLP's two layers, or the CNN's conv stack and linear layer
int encoder_forward(const Ctx& C) {
  int rc;
  if (C.L.enc == GO1_PPO_ENC_CNN) return (rc = launch_conv(C.s, C.conv(false))) ? rc : forward(C, W_CNN);
  return (rc = forward(C, W_E0)) ? rc : forward(C, W_E2);
}

// the CNN encoder below d emb: d feat = d emb W (its maximum with it), then the conv stack's backward
int conv_backward(const Ctx& C) {
  int rc = launch_xw(C.s, C.L.M, EPI_LIN, C.bwd_feat());
  return rc ? rc : launch_conv(C.s, C.conv(true));
}

// ------------------------------------------------------------------ the phases (the launch chain of the header)
int grad_phase0(const Ctx& C) {
  const Lay& L = C.L;
  const go1_ppo_bufs* b = C.b;
  if (!b->obs_history || !b->privileged_obs || !b->actions || !b->values || !b->advantages || !b->returns ||
      !b->actions_log_prob || !b->mu || !b->sigma || !b->idx || b->hist_ld < L.Hs)
    return fail(GO1_PPO_E_ARG, "go1_ppo_grad: storage tensors and idx are required");
  int rc;
  // the mini-batch rows (the max slots were cleared by the previous step's finalize_kernel, or are fresh)
  {
    const dim3 grid(std::min(cdiv(L.M, 16), GATHER_BLOCKS_MAX));
    if (L.enc)
      hipLaunchKernelGGL(gather_kernel<true>, grid, dim3(256), 0, C.s, gather_args(C));
    else
      hipLaunchKernelGGL(gather_kernel<false>, grid, dim3(256), 0, C.s, gather_args(C));
    PPO_TRY(hipGetLastError());
  }
  // ---- forward: the encoder on the last frame's map (ppo_cse_cnn: process_obs_history), once for the three heads:
  // e1 = ELU(W0 map + b0), emb = ELU(W1 e1 + b1) into G's leading E columns (its maximum into MX_LAT)
  // (the CNN: conv_kernel's features, then emb = W feat + b, no activation)
  if (L.enc && (rc = encoder_forward(C))) return rc;
  // ---- forward: adaptation module (ppo.py:110 ac.act -> update_distribution -> adaptation_module)
  if ((rc = forward(C, W_A0)) || (rc = forward(C, W_A2))) return rc;
  const AdaptArgs AD = adapt_args(C);
  hipLaunchKernelGGL(adapt_kernel<0>, dim3(L.HB), dim3(256), 0, C.s, AD);
  PPO_TRY(hipGetLastError());
  // ---- forward: actor [hist, latent] and critic [hist, latent (zero weights), priv]
  if ((rc = forward(C, W_P0, W_C0)) || (rc = forward(C, W_P2, W_C2)) || (rc = forward(C, W_P4, W_C4))) return rc;
  // ---- heads, loss, backward through L4 (ppo.py:111-155)
  if (L.A <= 12)
    hipLaunchKernelGGL(head_kernel<12>, dim3(L.HB), dim3(256), 0, C.s, head_args(C));
  else
    hipLaunchKernelGGL(head_kernel<16>, dim3(L.HB), dim3(256), 0, C.s, head_args(C));
  PPO_TRY(hipGetLastError());
  // ---- backward through L3, L2 (delta = W^T delta_next * ELU'(a))
  if ((rc = backward(C, W_P4, W_C4)) || (rc = backward(C, W_P2, W_C2))) return rc;
  // ---- the latent's gradient into the adaptation module, its L3 and L2 backward
  hipLaunchKernelGGL(adapt_kernel<2>, dim3(L.HB), dim3(256), 0, C.s, AD);
  PPO_TRY(hipGetLastError());
  if ((rc = backward(C, W_A2))) return rc;
  // ---- the embedding's gradient from the three first layers, then the encoder's hidden layer's
  if (L.enc) {
    const XwProb tp = C.bwd_lin(W_P0, L.tp), tc = C.bwd_lin(W_C0, L.tc);
    if ((rc = launch_xw(C.s, L.M, EPI_LIN, tp, &tc))) return rc;
    if ((rc = launch_xw(C.s, L.M, EPI_LIN, C.bwd_lin(W_A0, L.ta)))) return rc;
    hipLaunchKernelGGL(embgrad_kernel, dim3(L.MT, L.E / TB), dim3(256), 0, C.s, emb_args(C));
    PPO_TRY(hipGetLastError());
    if ((rc = L.enc == GO1_PPO_ENC_CNN ? conv_backward(C) : backward(C, W_E2))) return rc;
  }
  if ((rc = weight_grads(C, 0))) return rc;
  // ---- partials -> flat gradient (+ aux: surrogate, value, KL sums)
  SegBuilder SB;
  const int hs = head_stride(L.A), A = L.A;
  const HeadPart o(A);
  const float* hp = C.at<float>(L.hpart);
  SB.add(b->grads, hp + o.loss, 1, 3, 0, L.HB, hs);
  adapt_slice_segments(C, SB, 0);
  C.segs(SB, W_P0, 0);
  C.segs(SB, W_P2, 0);
  C.segs(SB, W_P4, 0);
  SB.add(C.gW(IP6), hp + o.dW4p, 1, A * 128, 0, L.HB, hs);
  SB.add(C.gB(IP6), hp + o.db4p, 1, A, 0, L.HB, hs);
  C.segs(SB, W_C0, 0);
  C.segs(SB, W_C2, 0);
  C.segs(SB, W_C4, 0);
  SB.add(C.gW(IC6), hp + o.dW4c, 1, 128, 0, L.HB, hs);
  SB.add(C.gB(IC6), hp + o.db4c, 1, 1, 0, L.HB, hs);
  SB.add(b->grads + NAUX + L.pstd, hp + o.dstd, 1, A, 0, L.HB, hs);
  return launch_reduce(C.s, SB);
}

int grad_phase1(const Ctx& C) {
  const Lay& L = C.L;
  int rc;
  // the gathered rows G are this mini-batch's (phase 0); the maxima phase 1 recomputes were cleared by step 0.
  // The encoder's weights moved in step 0: the embedding columns of G are computed again
  if (L.enc && (rc = encoder_forward(C))) return rc;
  if ((rc = forward(C, W_A0)) || (rc = forward(C, W_A2))) return rc;
  hipLaunchKernelGGL(adapt_kernel<1>, dim3(L.HB), dim3(256), 0, C.s, adapt_args(C));
  PPO_TRY(hipGetLastError());
  if ((rc = backward(C, W_A2))) return rc;
  // d emb = (W_A0[:, emb]^T delta1a) * ELU'(emb): the adaptation module is the only path here; then delta e1
  if (L.enc == GO1_PPO_ENC_CNN) {
    // the CNN's embedding has no activation: d emb = W_A0[:, emb]^T delta1a as it is (embgrad: its column sums and
    // maximum), then the conv stack
    if ((rc = launch_xw(C.s, L.M, EPI_LIN, C.bwd_lin(W_A0, L.ta)))) return rc;
    EmbArgs ea = emb_args(C);
    ea.nsrc = 1;
    hipLaunchKernelGGL(embgrad_kernel, dim3(L.MT, L.E / TB), dim3(256), 0, C.s, ea);
    PPO_TRY(hipGetLastError());
    if ((rc = conv_backward(C))) return rc;
  } else if (L.enc && ((rc = backward(C, W_A0)) || (rc = backward(C, W_E2)))) {
    return rc;
  }
  if ((rc = weight_grads(C, 1))) return rc;
  SegBuilder SB;
  const float* ap = C.at<float>(L.apart);
  SB.add(C.b->grads + 3, ap + AdaptPart(L.P).loss, 1, 2, 0, L.HB, adapt_stride(L.P));  // aux[3], aux[4]: loss sums
  adapt_slice_segments(C, SB, 1);
  return launch_reduce(C.s, SB);
}

int step_phase(const Ctx& C, int phase) {
  const Lay& L = C.L;
  const go1_ppo_bufs* b = C.b;
  if (!b->steps || !b->lr || !b->losses || !b->exp_avg || !b->exp_avg_sq || !b->ad_exp_avg || !b->ad_exp_avg_sq)
    return fail(GO1_PPO_E_ARG, "go1_ppo_step: Adam state, steps, lr and losses are required");
  const float* g = b->grads + NAUX;
  const int64_t n = phase == 0 ? L.np_total : L.np_adapt;
  if (phase == 0) {
    hipLaunchKernelGGL(norm_kernel, dim3(NORM_BLOCKS), dim3(256), 0, C.s, g, n, C.at<double>(L.normp));
    PPO_TRY(hipGetLastError());
  }
  Finalize F{};
  F.phase = phase;
  F.M = L.M;
  F.num_train = L.num_train;
  F.nsel_all = L.P;
  F.hyper = b->hyper;
  F.aux = b->grads;
  F.norm_part = C.at<double>(L.normp);
  F.lr = b->lr;
  F.steps = b->steps;
  F.losses = b->losses;
  F.scal = C.at<float>(L.scal) + 8 * phase;
  // phase 0 clears the maxima phase 1 recomputes (the outputs and deltas of the adaptation slice's layers) and the
  // weight maxima of the pack that follows; phase 1 clears every activation / gradient maximum (the next mini-batch)
  // and the slice's weight maxima
  bool act[MX_N] = {}, wts[W_N] = {};
  for (int w = 0; w < L.nW; ++w) {
    const Layer& y = L.layer[w];
    if (y.adapt) act[y.out.mx] = act[y.delta.mx] = true;
    wts[w] = phase == 0 || y.adapt;
  }
  if (L.enc == GO1_PPO_ENC_CNN) act[MX_FEAT] = act[MX_DFEAT] = true;  // phase 1 runs the conv stack again
  if (phase == 1) std::fill(act, act + MX_N, true);
  int nr = 0;
  auto runs = [&](uint32_t* base, const bool* on, int count) {  // the set slots as runs zero[i][0 .. nz[i])
    for (int i = 0; i < count; ++i) {
      if (!on[i]) continue;
      if (i == 0 || !on[i - 1]) {
        if (nr == 6) return false;
        F.zero[nr++] = base + i;
      }
      ++F.nz[nr - 1];
    }
    return true;
  };
  if (!runs(C.mx(0), act, MX_N) || !runs(C.wmax(0), wts, W_N))
    return fail(GO1_PPO_E_ARG, "go1_ppo_step: more than six runs of max slots to clear");
  for (int i = nr; i < 6; ++i) F.zero[i] = C.mx(MX_G);
  hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(256), 0, C.s, F);
  PPO_TRY(hipGetLastError());
  float* m1 = phase == 0 ? b->exp_avg : b->ad_exp_avg;
  float* m2 = phase == 0 ? b->exp_avg_sq : b->ad_exp_avg_sq;
  const int nblk = (int)((n + 255) / 256);
  hipLaunchKernelGGL(adam_kernel, dim3(nblk > 1024 ? 1024 : nblk), dim3(256), 0, C.s, b->params, g, m1, m2, n,
                     (const float*)F.scal);
  PPO_TRY(hipGetLastError());
  return pack_weights(C, phase == 1, false);
}

}  // namespace

extern "C" {

const char* go1_ppo_last_error(void) { return g_err.c_str(); }

int go1_ppo_abi_version(void) { return GO1_PPO_ABI_VERSION; }

void go1_ppo_abi_sizes(int64_t out[3]) {
  out[0] = sizeof(go1_ppo_dims);
  out[1] = sizeof(go1_ppo_hyper);
  out[2] = sizeof(go1_ppo_bufs);
}

int go1_ppo_param_count(const go1_ppo_dims* d, int64_t* total, int64_t* adaptation) {
  Lay L;
  std::string err;
  if (!make_layout(d, L, err)) return fail(GO1_PPO_E_ARG, err);
  if (total) *total = L.np_total;
  if (adaptation) *adaptation = L.np_adapt;
  return GO1_PPO_OK;
}

int go1_ppo_workspace_bytes(const go1_ppo_dims* d, int64_t* bytes) {
  Lay L;
  std::string err;
  if (!make_layout(d, L, err)) return fail(GO1_PPO_E_ARG, err);
  if (bytes) *bytes = (int64_t)L.total;
  return GO1_PPO_OK;
}

int go1_ppo_pack(const go1_ppo_dims* d, const go1_ppo_bufs* b, void* stream) {
  Ctx C;
  int rc = check_ctx(d, b, C, stream);
  if (rc) return rc;
  return pack_weights(C, false, true);
}

int go1_ppo_grad(const go1_ppo_dims* d, const go1_ppo_bufs* b, int32_t phase, void* stream) {
  // num_train = mb / 5 * 4 (ppo.py:165) is 0 below 5 rows: the adaptation loss would divide by zero (the layout
  // itself accepts mb >= 1: go1_ppo_param_count is asked with mb = 1)
  if (d && d->mb < 5)
    return fail(GO1_PPO_E_ARG, "go1_ppo_grad: mb >= 5 required (num_train = mb / 5 * 4 training rows, ppo.py:165)");
  Ctx C;
  int rc = check_ctx(d, b, C, stream);
  if (rc) return rc;
  if (phase == 0) return grad_phase0(C);
  if (phase == 1) return grad_phase1(C);
  return fail(GO1_PPO_E_ARG, "go1_ppo_grad: phase 0 or 1");
}

int go1_ppo_step(const go1_ppo_dims* d, const go1_ppo_bufs* b, int32_t phase, void* stream) {
  Ctx C;
  int rc = check_ctx(d, b, C, stream);
  if (rc) return rc;
  if (phase != 0 && phase != 1) return fail(GO1_PPO_E_ARG, "go1_ppo_step: phase 0 or 1");
  return step_phase(C, phase);
}

#ifdef PPO_STAMPS
extern "C" int go1_ppo_xw_stamps(void* host) {
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_xw_stamps), sizeof(g_xw_stamps), 0, hipMemcpyDeviceToHost) != hipSuccess;
}
#endif
// ---- test entry points: one GEMM of each kind on caller tensors (x rows 16-byte aligned: k % 4 == 0 or padded)
int go1_ppo_test_linear(const float* x, int64_t rows, int32_t k, const float* w, const float* bias, int32_t n,
                        int32_t elu, float* y, void* work, int64_t work_bytes, int32_t reps, void* stream) {
  if (!x || !w || !bias || !y || !work || rows < 1 || k < 1 || n < TB || n % TB != 0)
    return fail(GO1_PPO_E_ARG, "go1_ppo_test_linear: bad argument (n a multiple of 128)");
  const int G = cdiv(k, 32), ldx = cdiv(k, 4) * 4;
  const size_t need = 1024 + (size_t)G * 32 * n * 4 + (size_t)rows * ldx * 4;
  if ((size_t)work_bytes < need) return fail(GO1_PPO_E_ARG, "go1_ppo_test_linear: work too small");
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)work;
  uint32_t* mx = (uint32_t*)ws;  // [0] x max, [1] w max, [2] y max
  int32_t* wexp = (int32_t*)(ws + 64);
  h8_t* img = (h8_t*)(ws + 1024);
  float* xp = (float*)(ws + 1024 + (size_t)G * 32 * n * 4);  // x with rows padded to 16 bytes
  PPO_TRY(hipMemsetAsync(ws, 0, need, s));
  PPO_TRY(hipMemcpy2DAsync(xp, ldx * 4, x, (size_t)k * 4, (size_t)k * 4, rows, hipMemcpyDeviceToDevice, s));
  hipLaunchKernelGGL(absmax_kernel, dim3(256), dim3(256), 0, s, x, rows, k, (int64_t)k, mx);
  PackBuilder PB;
  PB.add(pack_w(w, n, k, img, mx + 1, wexp));
  int rc = launch_pack(s, PB);
  XwProb q = xw_prob(Opnd{xp, ldx, mx, nullptr}, k, img, wexp, n, y, n, mx + 2);
  q.bias = bias;
  for (int i = 0; !rc && i < (reps > 1 ? reps : 1); ++i) rc = launch_xw(s, (int)rows, elu ? EPI_ELU : EPI_LIN, q);
  return rc;
}

int go1_ppo_test_wgrad(const float* x, const float* d, int64_t rows, int32_t k, int32_t n, float* dw, void* work,
                       int64_t work_bytes, int32_t reps, void* stream) {
  if (!x || !d || !dw || !work || rows < 1 || k < 1 || n < TB || n % TB != 0)
    return fail(GO1_PPO_E_ARG, "go1_ppo_test_wgrad: bad argument (n a multiple of 128)");
  const int kpad = cdiv(k, TB) * TB, ldx = cdiv(k, 4) * 4;
  int S = (int)(cdiv((int)rows, TB) * TB / 256);
  S = S >= 16 ? 16 : (S >= 8 ? 8 : (S < 1 ? 1 : S));
  const int chunk = cdiv(cdiv((int)rows, S), 32) * 32;
  S = cdiv((int)rows, chunk);
  const size_t need = 1024 + (size_t)S * n * kpad * 4 + (size_t)rows * ldx * 4;
  if ((size_t)work_bytes < need) return fail(GO1_PPO_E_ARG, "go1_ppo_test_wgrad: work too small");
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)work;
  uint32_t* mx = (uint32_t*)ws;
  float* part = (float*)(ws + 1024);
  float* xp = part + (size_t)S * n * kpad;
  PPO_TRY(hipMemsetAsync(ws, 0, 1024, s));
  PPO_TRY(hipMemcpy2DAsync(xp, ldx * 4, x, (size_t)k * 4, (size_t)k * 4, rows, hipMemcpyDeviceToDevice, s));
  hipLaunchKernelGGL(absmax_kernel, dim3(256), dim3(256), 0, s, x, rows, k, (int64_t)k, mx);
  hipLaunchKernelGGL(absmax_kernel, dim3(256), dim3(256), 0, s, d, rows, n, (int64_t)n, mx + 1);
  const WgProb p = wg_prob(Opnd{xp, ldx, mx, nullptr}, k, Opnd{d, n, mx + 1, nullptr}, n, part);
  int rc = GO1_PPO_OK;
  for (int i = 0; !rc && i < (reps > 1 ? reps : 1); ++i) rc = launch_wg(s, (int)rows, S, chunk, &p, 1);
  if (rc) return rc;
  SegBuilder SB;
  SB.add(dw, part, n, k, kpad, S, p.pstride);
  return launch_reduce(s, SB);
}

// The CNN height-map encoder's convolution stack on `rows` maps (rows, 3782): feat (rows, 3360) and, for the loss
// gradient d_feat (rows, 3360) of the features, the filters' and biases' gradients summed over the rows
int go1_ppo_test_conv(const float* maps, int64_t rows, const float* w1, const float* b1, const float* w2,
                      const float* b2, const float* d_feat, float* feat, float* dw1, float* db1, float* dw2,
                      float* db2, void* work, int64_t work_bytes, int32_t reps, void* stream) {
  if (!maps || !w1 || !b1 || !w2 || !b2 || !d_feat || !feat || !dw1 || !db1 || !dw2 || !db2 || !work || rows < 1 ||
      rows > (1 << 24) || (((uintptr_t)work) & 255) != 0)
    return fail(GO1_PPO_E_ARG, "go1_ppo_test_conv: bad argument (work 256-byte aligned, 1 .. 2^24 rows)");
  const int nwg = conv_groups((int)rows);
  const size_t imgs = 256, parts = imgs + (size_t)CV_IMG_N * sizeof(h8_t);
  const size_t need = parts + (size_t)nwg * CV_PART * sizeof(float);
  if ((size_t)work_bytes < need)
    return fail(GO1_PPO_E_ARG, "go1_ppo_test_conv: work too small (" + std::to_string(need) + " bytes)");
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)work;
  ConvPack cp{w1, w2, (h8_t*)(ws + imgs), (int32_t*)ws};
  hipLaunchKernelGGL(conv_pack_kernel, dim3(1), dim3(256), 0, s, cp);
  PPO_TRY(hipGetLastError());
  ConvArgs a{};
  a.map = maps;
  a.ldm = CV_NMAP;
  a.dfeat = d_feat;
  a.ldd = CV_NFEAT;
  a.feat = feat;
  a.ldf = CV_NFEAT;
  a.featmax = nullptr;
  a.img = cp.img;
  a.wexp = cp.wexp;
  a.b1 = b1;
  a.b2 = b2;
  a.part = (float*)(ws + parts);
  a.rows = (int32_t)rows;
  a.strip = conv_strip((int)rows);
  int rc = GO1_PPO_OK;
  for (int i = 0; !rc && i < (reps > 1 ? reps : 1); ++i) rc = launch_conv(s, a);
  if (rc) return rc;
  SegBuilder SB;
  SB.add(dw2, a.part, 1, CV_C2 * CV_K2, 0, nwg, CV_PART);
  SB.add(db2, a.part + CV_OFF_DB2, 1, CV_C2, 0, nwg, CV_PART);
  SB.add(dw1, a.part + CV_OFF_DW1, 1, CV_C1 * CV_K1, 0, nwg, CV_PART);
  SB.add(db1, a.part + CV_OFF_DB1, 1, CV_C1, 0, nwg, CV_PART);
  return launch_reduce(s, SB);
}

}  // extern "C"

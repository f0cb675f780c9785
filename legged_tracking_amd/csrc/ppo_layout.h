// ppo_layout.h -- part of ppo_update.hip, host only: the max and weight slots, the parameter order, the workspace
// layout of a go1_ppo_dims and the table of the GEMM layers.  Every fact about a layer (its operands, their strides
// and max slots, whether phase 1 runs it, whether the backward crosses it) is stated once, as a row of that table;
// the image sizes, the pack list, the forward / backward / weight-gradient problems, the reduce segments and the max
// slots to clear are derived from the rows (Ctx).
#pragma once

namespace {

enum MaxSlot {
  MX_G = 0,  // the gathered mini-batch rows (obs_history, privileged_obs)
  MX_LAT, MX_A1A, MX_A2A, MX_P1, MX_P2, MX_P3, MX_C1, MX_C2, MX_C3,
  MX_D3P, MX_D3C, MX_D2P, MX_D2C, MX_D1P, MX_D1C, MX_D2A, MX_D1A,
  // the encoder: the gathered map, its hidden layer, d emb, d hidden.  The embedding's maximum goes to MX_LAT, the
  // slot of G's computed columns (embedding, latent): the first layers' scale max(MX_G, MX_LAT) bounds it
  MX_MAP, MX_E1, MX_DEMB, MX_DE1,
  // the CNN encoder: the conv stack's features (the input of its linear layer) and their gradient.  MX_DFEAT is a
  // record only (the issue's "max |d feat| in a new max slot"): no kernel scales by it, conv_kernel takes each row's
  // own maximum of d feat in LDS, which rows of mixed magnitude need
  MX_FEAT, MX_DFEAT,
  MX_N
};
// one weight image per GEMM layer: the adaptation module's, the actor's and the critic's first three, the MLP
// encoder's two
enum WSlot { W_A0 = 0, W_A2, W_P0, W_P2, W_P4, W_C0, W_C2, W_C4, W_E0, W_E2, W_N };
constexpr int W_PLAIN = W_E0;  // the slots of the plain module
// the CNN encoder has one GEMM layer, Linear(3360, E), in the slot W_E0 (the MLP's W_E2 is then unused); its two
// convolutions are conv_kernel's (ppo_conv.h), with their scale exponents in the two wexp records after the layers'
constexpr int W_CNN = W_E0, WEXP_CONV = W_N;
constexpr int ENC_H = GO1_PPO_ENC_HIDDEN;
constexpr int CV_DPAD = (CV_NFEAT + TB - 1) / TB * TB;  // d feat's row: 3360 padded to the xw tile, 3456
// parameter indices: a0 a2 a4 | p0 p2 p4 p6 | c0 c2 c4 c6 | the encoder's e0 e2 (first in the flat buffers)
enum { IA0 = 0, IA2, IA4, IP0, IP2, IP4, IP6, IC0, IC2, IC4, IC6, IE0, IE2 };

struct Mat {  // an activation or gradient buffer: workspace byte offset, row stride (floats), max slot
  size_t off;
  int ld, mx;
};
struct BiasSrc {  // where a bias gradient is summed from: nparts partial rows, pstride floats apart
  size_t off;
  int nparts;
  int64_t pstride;
};

// out = ELU(in W^T + b) with W of (n, k - gap) and `delta` the loss gradient before the ELU
struct Layer {
  int param;     // parameter index of W and b
  int n, k;      // output width (a multiple of TB); GEMM columns: the input's real columns
  Mat in;
  int in_mx2;    // the input's second max slot (G's computed columns), or -1
  Mat out, delta;
  BiasSrc bias;  // delta's column sums: an xw<D> launch's [MT][n], or a slice of the head / adapt partials
  int below;     // the layer whose output this one reads (as its leading columns): the backward crosses this layer's
                 // transposed image to reach that one's delta.  -1: the backward ends here (or takes another kernel)
  bool adapt;    // in the adaptation optimizer's slice: phase 1 runs it again
  bool first;    // reads the gathered rows G: with an encoder its image's columns are permuted (pack_kernel)
  bool lin;      // no activation: out = in W^T + b (the CNN encoder's linear layer)
  int kt_own;    // columns of a transposed image the layer needs although no table row is below it (0: none).  Columns
                 // past k are padding that the pack never writes: they are zero because the caller zeroes the
                 // workspace once before first use (go1_ppo.h), as the zero bias `zbias` is
  int gap;       // first layers: G columns at H that the parameter does not have (the critic skips the latent)
  // derived by make_layout: the transposed image's columns (0: none) and the workspace offsets
  int kt;
  size_t part, img, imgt;
  int kpad() const { return cdiv(k, TB) * TB; }  // row length of a weight-gradient partial [S][n][kpad]
};

struct Lay {
  int H, P, A, M, MP, MT, HB, ldg, bw;  // H: the heads' input width (hist; 2 SC + E with an encoder)
  int num_train;                        // rows of the adaptation loss: int(data_size // 5 * 4) (ppo.py:166)
  // the encoder (enc = 0: none): embedding width, scalars and map values of a frame, the map buffer's row stride,
  // the stored history width and the last frame's first column in it; nW: weight slots in use
  int enc, E, SC, NM, ldm, Hs, foff, nW;
  int S[2], chunk[2];  // weight-gradient row split per phase (about two workgroups per CU in one round)
  int64_t np_total, np_adapt;
  // parameter offsets (floats) in state_dict order
  int64_t pw[13], pb[13], pstd;  // indexed by IA0 .. IC6, IE0, IE2
  // workspace byte offsets: the records, then the buffers that kernels other than the GEMMs name
  size_t maxes, wmax, wexp, scal, normp, G, Bb, a2a, p3, c3, d3p, d3c, d1p, d2a, hpart, apart, total;
  size_t mapb, demb, tp, tc, ta, csemb, zbias;  // the encoder's
  int64_t pwc[2], pbc[2];                        // the CNN encoder's conv filters and biases (floats)
  size_t feat, dfeat, cvimg, cvpart;             // its features, their gradient, the filters' images, the partials
  int cvS, cvG;                                  // conv_kernel's strip and workgroups for mb rows
  Layer layer[W_N];
};

bool make_layout(const go1_ppo_dims* d, Lay& L, std::string& err) {
  if (!d || d->hist < 1 || d->priv < 1 || d->priv > 8 || d->actions < 1 || d->actions > 16 || d->mb < 1 ||
      d->rows < d->mb) {
    err = "go1_ppo: dims outside the supported architecture (hist >= 1, priv 1..8, actions 1..16, mb <= rows)";
    return false;
  }
  L = Lay{};
  L.enc = d->enc_mode;
  L.Hs = L.H = d->hist;
  L.nW = W_PLAIN;
  if (d->enc_mode != GO1_PPO_ENC_NONE) {
    const bool cnn = d->enc_mode == GO1_PPO_ENC_CNN;
    if (d->enc_mode != GO1_PPO_ENC_MLP && !cnn) {
      err = "go1_ppo: enc_mode " + std::to_string(d->enc_mode) + " is not implemented (0: no encoder, 1: the MLP "
            "encoder, 3: the CNN encoder on the (2, 61, 31) map)";
      return false;
    }
    if (d->n_embed < TB || d->n_embed % TB != 0 || d->n_embed > GO1_PPO_ENC_MAX_EMBED) {
      err = "go1_ppo: n_embed " + std::to_string(d->n_embed) + " is not implemented (a multiple of 128, at most 512)";
      return false;
    }
    if (d->n_map < 1 || d->n_map > GO1_PPO_ENC_MAX_MAP || d->n_map > d->num_obs) {
      err = "go1_ppo: n_map " + std::to_string(d->n_map) + " is not implemented (1..4096 map values, at most num_obs)";
      return false;
    }
    if (cnn && d->n_map != CV_NMAP) {
      err = "go1_ppo: n_map " + std::to_string(d->n_map) + " is not implemented with the CNN encoder (3782: the (2, 61, "
            "31) map, whose twice-pooled size is the encoder's Linear(3360, E))";
      return false;
    }
    if (d->hist % d->num_obs != 0) {
      err = "go1_ppo: hist " + std::to_string(d->hist) + " is not a multiple of num_obs " + std::to_string(d->num_obs) +
            " (whole frames; the encoder reads the last one)";
      return false;
    }
    L.E = d->n_embed;
    L.NM = d->n_map;
    L.SC = d->num_obs - d->n_map;
    L.H = 2 * L.SC + L.E;
    L.foff = d->hist - d->num_obs;
    L.ldm = cdiv(L.NM, 4) * 4;
    L.nW = cnn ? W_CNN + 1 : W_N;
  }
  const bool cnn = L.enc == GO1_PPO_ENC_CNN;
  L.P = d->priv;
  L.A = d->actions;
  L.M = d->mb;
  L.num_train = (L.M / 5) * 4;
  L.MT = cdiv(L.M, TB);
  L.MP = L.MT * TB;
  L.HB = std::min(HEAD_BLOCKS, cdiv(L.M, 4));
  L.ldg = cdiv(L.H + 2 * L.P, 4) * 4;  // [hist, latent, priv]
  L.bw = cdiv(3 * L.A + 4, 4) * 4;     // [actions, mu, sigma, logp, adv, ret, values]
  // parameters
  const int H = L.H, P = L.P, A = L.A, E = L.E, MT = L.MT, ldg = L.ldg;
  const int64_t wsz[11] = {(int64_t)HA1 * H, HA2 * HA1, P * HA2, (int64_t)H1 * (H + P), H2 * H1, H3 * H2, A * H3,
                           (int64_t)H1 * (H + P), H2 * H1, H3 * H2, 1 * H3};
  const int64_t bsz[11] = {HA1, HA2, P, H1, H2, H3, A, H1, H2, H3, 1};
  int64_t o = 0;
  if (cnn) {  // [conv1 w, b | conv2 w, b | linear w, b], the module's order
    const int64_t csz[2] = {CV_C1 * CV_K1, CV_C2 * CV_K2}, cb[2] = {CV_C1, CV_C2};
    for (int i = 0; i < 2; ++i) {
      L.pwc[i] = o;
      o += csz[i];
      L.pbc[i] = o;
      o += cb[i];
    }
    L.pw[IE2] = o;
    o += (int64_t)E * CV_NFEAT;
    L.pb[IE2] = o;
    o += E;
  } else if (L.enc) {  // the encoder leads the flat buffers: the adaptation optimizer's slice is encoder + adaptation module
    L.pw[IE0] = o;
    o += (int64_t)ENC_H * L.NM;
    L.pb[IE0] = o;
    o += ENC_H;
    L.pw[IE2] = o;
    o += (int64_t)E * ENC_H;
    L.pb[IE2] = o;
    o += E;
  }
  for (int i = 0; i < 11; ++i) {
    L.pw[i] = o;
    o += wsz[i];
    L.pb[i] = o;
    o += bsz[i];
    if (i == IA4) L.np_adapt = o;
  }
  L.pstd = o;
  o += A;
  L.np_total = o;
  // workspace
  size_t b = 0;
  auto take = [&](size_t bytes) {
    const size_t at = b;
    b += (bytes + 255) & ~(size_t)255;
    return at;
  };
  const size_t F = sizeof(float), MPs = (size_t)L.MP;
  auto rows = [&](int cols) { return take(MPs * cols * F); };       // an [MP][cols] activation / gradient
  auto sums = [&](int cols) { return take((size_t)MT * cols * F); };  // an xw<D> launch's [MT][cols] column sums
  L.maxes = take(64 * 4);
  L.wmax = take(16 * 4);
  L.wexp = take(16 * 4);
  L.scal = take(32 * 4);
  L.normp = take(NORM_BLOCKS * 8);
  // the buffers that kernels other than the GEMMs name; a buffer only the GEMMs touch is taken in its table row
  L.G = rows(ldg);
  L.Bb = rows(L.bw);
  L.a2a = rows(HA2);
  L.p3 = rows(H3);
  L.c3 = rows(H3);
  L.d3p = rows(H3);
  L.d3c = rows(H3);
  L.d1p = rows(H1);
  L.d2a = rows(HA2);
  L.hpart = take((size_t)HEAD_BLOCKS * head_stride(A) * F);
  L.apart = take((size_t)ADAPT_BLOCKS * adapt_stride(P) * F);
  if (L.enc) {
    L.mapb = rows(L.ldm);
    L.demb = rows(E);
    L.tp = rows(E);
    L.tc = rows(E);
    L.ta = rows(E);
    L.csemb = sums(E);
    // zeros (never written): the bias of the xw<LIN> products
    L.zbias = take((size_t)(cnn ? CV_DPAD : GO1_PPO_ENC_MAX_EMBED) * F);
  }
  if (cnn) {
    L.feat = rows(CV_NFEAT);
    L.dfeat = rows(CV_DPAD);
    L.cvimg = take((size_t)CV_IMG_N * sizeof(h8_t));
    L.cvS = conv_strip(L.M);
    L.cvG = conv_groups(L.M);
    L.cvpart = take((size_t)L.cvG * CV_PART * F);
  }
  // ---- the layer table.  A layer reads the output of the layer below it (input {}: filled in from `below`), except
  // the first layers, which read the gathered rows: the actor G's [hist, latent], the critic [hist, latent, priv] with
  // zero weights on the latent columns (its gap), the adaptation module [hist]; with an encoder G's leading E columns
  // are the embedding, the output of W_E2, which all three first layers read (`emb`) and whose maximum is G's second
  // (`lat`).  The last layers' deltas come from head_kernel / adapt_kernel, and their bias sums with them.
  const int hs = head_stride(A), as = adapt_stride(P), HB = L.HB;
  const HeadPart hp(A);
  const AdaptPart ap(P);
  const int lat = L.enc ? MX_LAT : -1, emb = cnn ? W_CNN : (L.enc ? W_E2 : -1);
  const Mat G = {L.G, ldg, MX_G};
  Layer* T = L.layer;
  //         param n   k   input max2   output                   delta                    bias sums
  //         below adapt first gap
  T[W_A0] = {IA0, HA1, H, G, lat, {rows(HA1), HA1, MX_A1A}, {rows(HA1), HA1, MX_D1A}, {sums(HA1), MT, HA1},
             emb, true, true, false, 0, 0};
  T[W_A2] = {IA2, HA2, HA1, {}, -1, {L.a2a, HA2, MX_A2A}, {L.d2a, HA2, MX_D2A}, {L.apart + ap.db2a * F, HB, as},
             W_A0, true, false, false, 0, 0};
  T[W_P0] = {IP0, H1, H + P, G, MX_LAT, {rows(H1), H1, MX_P1}, {L.d1p, H1, MX_D1P}, {sums(H1), MT, H1},
             emb, false, true, false, 0, 0};
  T[W_P2] = {IP2, H2, H1, {}, -1, {rows(H2), H2, MX_P2}, {rows(H2), H2, MX_D2P}, {sums(H2), MT, H2},
             W_P0, false, false, false, 0, 0};
  T[W_P4] = {IP4, H3, H2, {}, -1, {L.p3, H3, MX_P3}, {L.d3p, H3, MX_D3P}, {L.hpart + hp.db3p * F, HB, hs},
             W_P2, false, false, false, 0, 0};
  T[W_C0] = {IC0, H1, H + 2 * P, G, MX_LAT, {rows(H1), H1, MX_C1}, {rows(H1), H1, MX_D1C}, {sums(H1), MT, H1},
             emb, false, true, false, 0, P};
  T[W_C2] = {IC2, H2, H1, {}, -1, {rows(H2), H2, MX_C2}, {rows(H2), H2, MX_D2C}, {sums(H2), MT, H2},
             W_C0, false, false, false, 0, 0};
  T[W_C4] = {IC4, H3, H2, {}, -1, {L.c3, H3, MX_C3}, {L.d3c, H3, MX_D3C}, {L.hpart + hp.db3c * F, HB, hs},
             W_C2, false, false, false, 0, 0};
  if (cnn) {  // emb = feat W^T + b, no activation, into G; the conv stack below it is conv_kernel's, which takes
              // d feat = d emb W: the transposed image of all 3360 columns, padded to the tile with zero columns
    T[W_CNN] = {IE2, E, CV_NFEAT, {L.feat, CV_NFEAT, MX_FEAT}, -1, {L.G, ldg, MX_LAT}, {L.demb, E, MX_DEMB},
                {L.csemb, MT, E}, -1, true, false, true, CV_DPAD, 0};
  } else if (L.enc) {
    T[W_E0] = {IE0, ENC_H, L.NM, {L.mapb, L.ldm, MX_MAP}, -1, {rows(ENC_H), ENC_H, MX_E1},
               {rows(ENC_H), ENC_H, MX_DE1}, {sums(ENC_H), MT, ENC_H}, -1, true, false, false, 0, 0};
    T[W_E2] = {IE2, E, ENC_H, {}, -1, {L.G, ldg, MX_LAT}, {L.demb, E, MX_DEMB}, {L.csemb, MT, E},
               W_E0, true, false, false, 0, 0};
  }
  for (int w = 0; w < L.nW; ++w)
    if (!T[w].first && T[w].below >= 0) T[w].in = T[T[w].below].out;
  // the row split of each phase's grouped weight-gradient launch: at most 512 workgroups (two per CU with the
  // launch's 64 KiB of LDS: one more would start a second round), chunks of >= 64 rows
  int tiles[2] = {0, 0};
  for (int w = 0; w < L.nW; ++w) {
    const int t = T[w].kpad() / TB * (T[w].n / TB);
    tiles[0] += t;
    if (T[w].adapt) tiles[1] += t;
  }
  for (int ph = 0; ph < 2; ++ph) {
    int S = 512 / tiles[ph];
    S = std::max(1, std::min(std::min(S, 64), L.M / 64));
    L.chunk[ph] = cdiv(cdiv(L.M, S), 32) * 32;
    L.S[ph] = cdiv(L.M, L.chunk[ph]);
  }
  // weight-gradient partials [S][n][kpad] and weight images (4 bytes per element: hi + lo halves), the transposed
  // one of the columns the backward needs: the width of the layer below
  for (int w = 0; w < L.nW; ++w) {
    Layer& y = T[w];
    const int S = y.adapt ? std::max(L.S[0], L.S[1]) : L.S[0];
    y.kt = y.below >= 0 ? T[y.below].n : y.kt_own;
    y.part = take((size_t)S * y.n * y.kpad() * F);
    y.img = take((size_t)cdiv(y.k, 32) * 32 * y.n * 4);
    y.imgt = y.kt ? take((size_t)cdiv(y.n, 32) * 32 * y.kt * 4) : 0;
  }
  L.total = b;
  return true;
}

// One call's view of the buffers: the caller's tensors, the workspace, and the problems of a layer.
struct Ctx {
  const go1_ppo_dims* d;
  const go1_ppo_bufs* b;
  Lay L;
  char* ws;
  hipStream_t s;
  template <class T>
  T* at(size_t off) const {
    return reinterpret_cast<T*>(ws + off);
  }
  uint32_t* mx(int slot) const { return at<uint32_t>(L.maxes) + slot; }
  uint32_t* wmax(int w) const { return at<uint32_t>(L.wmax) + w; }
  int32_t* wexp(int w) const { return at<int32_t>(L.wexp) + w; }
  const float* W(int i) const { return b->params + L.pw[i]; }
  const float* B(int i) const { return b->params + L.pb[i]; }
  float* gW(int i) const { return b->grads + NAUX + L.pw[i]; }
  float* gB(int i) const { return b->grads + NAUX + L.pb[i]; }
  Opnd opnd(const Mat& m, int mx2 = -1) const {
    return {at<float>(m.off), m.ld, mx(m.mx), mx2 >= 0 ? mx(mx2) : nullptr};
  }

  // the image(s) of layer w from its parameter
  PackW pack(int w) const {
    const Layer& y = L.layer[w];
    PackW p = pack_w(W(y.param), y.n, y.k, at<h8_t>(y.img), wmax(w), wexp(w));
    p.ldw = y.k - y.gap;
    p.gap_at = y.gap ? L.H : 0;
    p.gap = y.gap;
    if (L.enc && y.first) p.perm_e = L.E, p.perm_p = L.H;
    if (y.kt) p.imgt = at<h8_t>(y.imgt), p.npadt = y.kt;
    return p;
  }
  // forward: out = act(in W^T + b)
  XwProb fwd(int w) const {
    const Layer& y = L.layer[w];
    XwProb p = xw_prob(opnd(y.in, y.in_mx2), y.k, at<h8_t>(y.img), wexp(w), y.n, at<float>(y.out.off), y.out.ld,
                       mx(y.out.mx));
    p.bias = B(y.param);
    return p;
  }
  // backward across w: the delta of the layer below, (delta W) * ELU'(its output), and its column sums
  XwProb bwd(int w) const {
    const Layer &y = L.layer[w], &u = L.layer[y.below];
    XwProb p = xw_prob(opnd(y.delta), y.n, at<h8_t>(y.imgt), wexp(w), u.n, at<float>(u.delta.off), u.delta.ld,
                       mx(u.delta.mx));
    p.aprev = at<float>(u.out.off);
    p.ldp = u.out.ld;
    p.colsum = at<float>(u.bias.off);
    return p;
  }
  // the plain product delta W[:, embedding] of a first layer into `out` ([M][E]: embgrad_kernel sums the three)
  XwProb bwd_lin(int w, size_t out) const {
    const Layer& y = L.layer[w];
    XwProb p = xw_prob(opnd(y.delta), y.n, at<h8_t>(y.imgt), wexp(w), y.kt, at<float>(out), y.kt, nullptr);
    p.bias = at<float>(L.zbias);
    return p;
  }
  // the CNN encoder: d feat = d emb W of its linear layer, [M][3456], and its maximum (a record: MaxSlot).  The last 96
  // columns come from the image's padding (zero with the workspace, Layer::kt_own); conv_kernel reads 3360 of a row
  XwProb bwd_feat() const {
    const Layer& y = L.layer[W_CNN];
    XwProb p = xw_prob(opnd(y.delta), y.n, at<h8_t>(y.imgt), wexp(W_CNN), y.kt, at<float>(L.dfeat), y.kt, mx(MX_DFEAT));
    p.bias = at<float>(L.zbias);
    return p;
  }
  // its conv stack on the gathered maps: the features (and their maximum) alone, or the filters' gradient partials too
  ConvPack conv_pack() const {
    return {b->params + L.pwc[0], b->params + L.pwc[1], at<h8_t>(L.cvimg), wexp(WEXP_CONV)};
  }
  ConvArgs conv(bool backward) const {
    ConvArgs a{};
    a.map = at<float>(L.mapb);
    a.ldm = L.ldm;
    a.dfeat = backward ? at<float>(L.dfeat) : nullptr;
    a.ldd = CV_DPAD;
    a.feat = backward ? nullptr : at<float>(L.feat);
    a.ldf = CV_NFEAT;
    a.featmax = backward ? nullptr : mx(MX_FEAT);
    a.img = at<h8_t>(L.cvimg);
    a.wexp = wexp(WEXP_CONV);
    a.b1 = b->params + L.pbc[0];
    a.b2 = b->params + L.pbc[1];
    a.part = at<float>(L.cvpart);
    a.rows = L.M;
    a.strip = L.cvS;
    return a;
  }
  void conv_segs(SegBuilder& SB) const {
    const float* pt = at<float>(L.cvpart);
    float* g = b->grads + NAUX;
    SB.add(g + L.pwc[0], pt + CV_OFF_DW1, 1, CV_C1 * CV_K1, 0, L.cvG, CV_PART);
    SB.add(g + L.pbc[0], pt + CV_OFF_DB1, 1, CV_C1, 0, L.cvG, CV_PART);
    SB.add(g + L.pwc[1], pt, 1, CV_C2 * CV_K2, 0, L.cvG, CV_PART);
    SB.add(g + L.pbc[1], pt + CV_OFF_DB2, 1, CV_C2, 0, L.cvG, CV_PART);
  }
  // weight gradient: partials of delta^T in
  WgProb wg(int w) const {
    const Layer& y = L.layer[w];
    return wg_prob(opnd(y.in, y.in_mx2), y.k, opnd(y.delta), y.n, at<float>(y.part));
  }
  // the layer's weight and bias gradient from their partials.  A first layer's partial has the image's columns, G's:
  // [embedding | scalars | scalars] against the parameter's [scalars | scalars | embedding] with an encoder, then the
  // columns past H (the actor's latent; the critic's priv, past its gap)
  void segs(SegBuilder& SB, int w, int phase) const {
    const Layer& y = L.layer[w];
    const int kpad = y.kpad(), ldd = y.k - y.gap;
    auto cols = [&](int dst, int src, int n) {
      if (n > 0)
        SB.add(gW(y.param) + dst, at<float>(y.part) + src, y.n, n, kpad, L.S[phase], (int64_t)y.n * kpad, ldd);
    };
    if (!y.first) {
      cols(0, 0, y.k);
    } else {
      if (L.enc) {
        cols(0, L.E, 2 * L.SC);
        cols(2 * L.SC, 0, L.E);
      } else {
        cols(0, 0, L.H);
      }
      cols(L.H, L.H + y.gap, ldd - L.H);
    }
    SB.add(gB(y.param), at<float>(y.bias.off), 1, y.n, 0, y.bias.nparts, y.bias.pstride);
  }
};

}  // namespace

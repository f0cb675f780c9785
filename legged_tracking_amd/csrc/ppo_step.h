// ppo_step.h -- part of ppo_update.hip: what turns partials into an optimizer step.  reduce_kernel (partials ->
// flat gradient) with its segment table, norm / finalize / adam, the weight maxima and the f16 fragment images
// (wmax / pack) with their table, absmax and zero.
#pragma once

namespace {

constexpr int NORM_BLOCKS = 256;

// ------------------------------------------------------------------ reduce: dst[r][c] = sum_p src[p][r][c]
// Segment table over every gradient tensor (and the aux sums); 256 threads per 64 output elements, the
// partials split four ways across the waves, summed in a fixed order.
struct Seg {
  float* dst;
  const float* src;
  int64_t lds, pstride, ldd;          // source row stride, partial stride, destination row stride
  int32_t rows, cols, nparts, start;  // start: first flat element of the segment in the launch
};
constexpr int MAX_SEGS = 40;  // phase 0 with an encoder: 33
struct SegTable {
  Seg s[MAX_SEGS];
  int32_t nseg, total;
};

__global__ __launch_bounds__(256) void reduce_kernel(SegTable T) {
  __shared__ float red[4][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int e = blockIdx.x * 64 + lane;
  float acc = 0.0f;
  int si = -1, r = 0, cc = 0;
  if (e < T.total) {
    si = 0;
    for (int i = 1; i < T.nseg; ++i)
      if (e >= T.s[i].start) si = i;
    const Seg& S = T.s[si];
    const int le = e - S.start;
    r = le / S.cols;
    cc = le - r * S.cols;
    const float* src = S.src + (size_t)r * S.lds + cc;
    // parts w, w + 4, w + 8, ...: eight independent chains (loads in flight), summed in a fixed order
    float a[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    int p = w;
    for (; p + 28 < S.nparts; p += 32)
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] += src[(size_t)(p + 4 * j) * S.pstride];
    for (int j = 0; p < S.nparts; p += 4, ++j) a[j & 7] += src[(size_t)p * S.pstride];
    acc = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
  }
  red[w][lane] = acc;
  __syncthreads();
  if (w == 0 && si >= 0) {
    const Seg& S = T.s[si];
    S.dst[(size_t)r * S.ldd + cc] = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
  }
}

struct SegBuilder {
  SegTable T{};
  void add(float* dst, const float* src, int rows, int cols, int64_t lds, int nparts, int64_t pstride,
           int64_t ldd = -1) {
    if (T.nseg++ >= MAX_SEGS) return;  // counted, not stored: launch_reduce reports the overflow
    Seg& s = T.s[T.nseg - 1];
    s.dst = dst;
    s.src = src;
    s.rows = rows;
    s.cols = cols;
    s.lds = lds;
    s.ldd = ldd < 0 ? cols : ldd;
    s.nparts = nparts;
    s.pstride = pstride;
    s.start = T.total;
    T.total += rows * cols;
  }
};

int launch_reduce(hipStream_t s, const SegBuilder& B) {
  if (B.T.nseg > MAX_SEGS) return fail(GO1_PPO_E_ARG, "go1_ppo: segment table overflow");
  hipLaunchKernelGGL(reduce_kernel, dim3(cdiv(B.T.total, 64)), dim3(256), 0, s, B.T);
  PPO_TRY(hipGetLastError());
  return GO1_PPO_OK;
}

// ------------------------------------------------------------------ norm, finalize, Adam
__global__ __launch_bounds__(256) void norm_kernel(const float* __restrict__ g, int64_t n, double* __restrict__ part) {
  __shared__ double red[256];
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const double v = g[i];
    s += v * v;
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

// Adam scalars for one optimiser step, written by finalize_kernel: [0] gradient scale (clip / world), [1] -step
// size, [2] sqrt(bias correction 2), [3] eps, [4] 1 - beta1, [5] beta2, [6] 1 - beta2
struct Finalize {
  int32_t phase, M, num_train, nsel_all;
  const go1_ppo_hyper* hyper;
  const float* aux;
  const double* norm_part;
  double* lr;
  float* steps;
  double* losses;
  float* scal;
  uint32_t* zero[6];  // max slots to clear for the launches that follow: zero[i][0 .. nz[i])
  int32_t nz[6];
};

__global__ __launch_bounds__(256) void finalize_kernel(Finalize F) {
  __shared__ double red[256];
  const go1_ppo_hyper hp = *F.hyper;
  const double world = hp.world > 0.0f ? (double)hp.world : 1.0;
#pragma unroll
  for (int i = 0; i < 6; ++i)
    if ((int)threadIdx.x < F.nz[i]) F.zero[i][threadIdx.x] = 0u;
  double s = 0.0;
  if (F.phase == 0) s = F.norm_part[threadIdx.x];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  double lr;
  float gscale;
  if (F.phase == 0) {
    // adaptive learning rate (ppo.py:119-132) from the KL mean over every rank's rows
    const float kl_mean = (float)((double)F.aux[2] / world) / (float)F.M;
    lr = F.lr[0];
    if (hp.desired_kl > 0.0f) {
      const double dk = (double)hp.desired_kl, k = (double)kl_mean;
      if (k > dk * 2.0)
        lr = fmax(1e-5, lr / 1.5);
      else if (k < dk / 2.0 && k > 0.0)
        lr = fmin(1e-2, lr * 1.5);
      F.lr[0] = lr;
    }
    // clip_grad_norm_ (ppo.py:157) of the rank-averaged gradient: clip_coef = max_norm / (norm + 1e-6), <= 1
    const float total = (float)(sqrt(red[0]) / world);
    const float coef = hp.max_grad_norm / (total + 1.0e-6f);
    gscale = (float)((double)fminf(coef, 1.0f) / world);
    F.losses[0] += (double)((float)((double)F.aux[1] / world) / (float)F.M);  // value loss
    F.losses[1] += (double)((float)((double)F.aux[0] / world) / (float)F.M);  // surrogate loss
  } else {
    lr = (double)hp.adaptation_lr;
    gscale = (float)(1.0 / world);
    const int nsel = hp.selective != 0.0f ? 1 : F.nsel_all;
    F.losses[2] += (double)((float)((double)F.aux[3] / world) / (float)(F.num_train * nsel));
    const int ntest = F.M - F.num_train;
    F.losses[3] += ntest > 0 ? (double)((float)((double)F.aux[4] / world) / (float)(ntest * nsel)) : 0.0;
  }
  // torch Adam (single-tensor form): step += 1; bias_correction1 = 1 - beta1 ** step; step_size = lr / bc1;
  // denom = sqrt(exp_avg_sq) / sqrt(bc2) + eps
  const float step = F.steps[F.phase] + 1.0f;
  F.steps[F.phase] = step;
  // The betas arrive as f32, and 1 - (double)0.999f is 1.3e-5 (relative) off torch's 1 - 0.999, 1 - (double)0.9f
  // 2.4e-7 off 1 - 0.9: the moments would drift from torch.optim.Adam's by that much.  Betas are decimal literals:
  // the double nearest to the f32's 7-significant-digit decimal is the Python float torch computes with (the
  // f32 spacing below 1 is finer than 1e-7, so the decimal is unambiguous; any other beta moves by < 5e-8).
  const double b1 = rint((double)hp.beta1 * 1.0e7) / 1.0e7, b2 = rint((double)hp.beta2 * 1.0e7) / 1.0e7;
  const double bc1 = 1.0 - pow(b1, (double)step), bc2 = 1.0 - pow(b2, (double)step);
  F.scal[0] = gscale;
  F.scal[1] = (float)(-(lr / bc1));
  F.scal[2] = (float)sqrt(bc2);
  F.scal[3] = hp.eps;
  F.scal[4] = (float)(1.0 - b1);
  F.scal[5] = (float)b2;
  F.scal[6] = (float)(1.0 - b2);
}

__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m1, float* __restrict__ m2, int64_t n,
                                                   const float* __restrict__ scal) {
  const float gs = scal[0], nss = scal[1], bc2s = scal[2], eps = scal[3], w1 = scal[4], b2 = scal[5], c2 = scal[6];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float gr = g[i] * gs;
    float a = m1[i];
    a = a + w1 * (gr - a);             // exp_avg.lerp_(grad, 1 - beta1)
    float v = m2[i] * b2;              // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    v = v + (c2 * gr) * gr;
    const float den = sqrtf(v) / bc2s + eps;
    p[i] = p[i] + (nss * a) / den;     // param.addcdiv_(exp_avg, denom, value=-step_size)
    m1[i] = a;
    m2[i] = v;
  }
}

// ------------------------------------------------------------------ weight max and the fragment images
struct PackW {
  const float* w;  // source (n, k - gap) with row stride ldw; image column kk reads source column kk (kk < gap_at),
                   // nothing (gap_at <= kk < gap_at + gap: zero weights), kk - gap (beyond)
  int32_t n, k, ldw, gap_at, gap, G, npad;
  // the encoder module's first layers: the image's (and G's) leading perm_p columns are [embedding perm_e | scalars],
  // the source's [scalars | embedding]; perm_p = 0: none
  int32_t perm_e, perm_p;
  h8_t* img;       // forward image [G][2][4][npad][8]
  h8_t* imgt;      // transposed image [ceil(n / 32)][2][4][npadt][8] of the image's first npadt columns, or NULL
  int32_t Gt, npadt;
  uint32_t* wmax;
  int32_t* wexp;
  int32_t start;   // first element of this tensor in the launch
};
constexpr int MAX_PACK = 10;
struct PackTable {
  PackW t[MAX_PACK];
  int32_t nt, total;
};

// grid (blocks, tensors): block-level max, one atomic per block and tensor
__global__ __launch_bounds__(256) void wmax_kernel(PackTable T) {
  __shared__ uint32_t red[4];
  const PackW& W = T.t[blockIdx.y];
  const int ks = W.k - W.gap, n = W.n * ks;
  uint32_t mx = 0u;
  for (int e = blockIdx.x * 256 + threadIdx.x; e < n; e += gridDim.x * 256) {
    const int r = e / ks;
    mx = max(mx, absbits(W.w[(size_t)r * W.ldw + (e - r * ks)]));
  }
  mx = wave_max_u32(mx);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    mx = max(max(red[0], red[1]), max(red[2], red[3]));
    if (mx) atomicMax(W.wmax, mx);
  }
}

__global__ __launch_bounds__(256) void pack_kernel(PackTable T) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= T.total) return;
  int ti = 0;
  for (int i = 1; i < T.nt; ++i)
    if (e >= T.t[i].start) ti = i;
  const PackW& W = T.t[ti];
  const int le = e - W.start, n = le / W.k, k = le - n * W.k;
  const int es = scale_exp(*W.wmax);
  if (le == 0) *W.wexp = es;
  const bool in_gap = k >= W.gap_at && k < W.gap_at + W.gap;
  int ks = k < W.gap_at ? k : k - W.gap;
  if (ks < W.perm_p) ks = ks < W.perm_e ? ks + (W.perm_p - W.perm_e) : ks - W.perm_e;
  const float x = in_gap ? 0.0f : ldexpf(W.w[(size_t)n * W.ldw + ks], es);
  const _Float16 hi = (_Float16)__builtin_amdgcn_cvt_pkrtz(x, 0.0f)[0];
  const _Float16 lo = (_Float16)__builtin_amdgcn_cvt_pkrtz(x - (float)hi, 0.0f)[0];
  {
    const int g = k >> 5, q = (k >> 3) & 3, r = k & 7;
    _Float16* base = reinterpret_cast<_Float16*>(W.img);
    base[(((size_t)(g * 2 + 0) * 4 + q) * W.npad + n) * 8 + r] = hi;
    base[(((size_t)(g * 2 + 1) * 4 + q) * W.npad + n) * 8 + r] = lo;
  }
  if (W.imgt && k < W.npadt) {
    const int g = n >> 5, q = (n >> 3) & 3, r = n & 7;
    _Float16* base = reinterpret_cast<_Float16*>(W.imgt);
    base[(((size_t)(g * 2 + 0) * 4 + q) * W.npadt + k) * 8 + r] = hi;
    base[(((size_t)(g * 2 + 1) * 4 + q) * W.npadt + k) * 8 + r] = lo;
  }
}

// host: the forward image of a dense (n, k) weight (no gap, no column map, no transposed image: the caller's to add)
PackW pack_w(const float* w, int n, int k, h8_t* img, uint32_t* wmax, int32_t* wexp) {
  PackW p{};
  p.w = w;
  p.n = n;
  p.k = k;
  p.ldw = k;
  p.G = cdiv(k, 32);
  p.npad = n;
  p.Gt = cdiv(n, 32);
  p.img = img;
  p.wmax = wmax;
  p.wexp = wexp;
  return p;
}

struct PackBuilder {
  PackTable T{};
  void add(PackW p) {
    p.start = T.total;
    T.total += p.n * p.k;
    T.t[T.nt++] = p;
  }
};

// the tensors' maxima (their records cleared by the caller), then their images
int launch_pack(hipStream_t s, const PackBuilder& B) {
  hipLaunchKernelGGL(wmax_kernel, dim3(32, B.T.nt), dim3(256), 0, s, B.T);
  PPO_TRY(hipGetLastError());
  hipLaunchKernelGGL(pack_kernel, dim3(cdiv(B.T.total, 256)), dim3(256), 0, s, B.T);
  PPO_TRY(hipGetLastError());
  return GO1_PPO_OK;
}

__global__ __launch_bounds__(256) void absmax_kernel(const float* __restrict__ x, int64_t rows, int32_t cols,
                                                     int64_t ld, uint32_t* __restrict__ out) {
  uint32_t mx = 0u;
  const int64_t total = rows * (int64_t)cols;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / cols;
    mx = max(mx, absbits(x[r * ld + (i - r * cols)]));
  }
  mx = wave_max_u32(mx);
  if ((threadIdx.x & 63) == 0) atomicMax(out, mx);
}

__global__ void zero_u32_kernel(uint32_t* p, int n) {
  if ((int)threadIdx.x < n) p[threadIdx.x] = 0u;
}

}  // namespace

// Inverted-residual (MBConv) block of the EfficientUnet++ decoder, inference form, NHWC fp32
// (reference: network/extra/efficientunetplusplus/decoder.py InvertedResidual — 1x1 conv, BN, Hardswish, depthwise 3x3,
// BN, Hardswish, scSE, 1x1 conv, BN, plus the input or a 1x1 + BN projection of it).
//
// A block is four or five launches and no element-wise pass over a mid-channel activation:
//   pwconv (Hardswish epilogue) -> dwconv (Hardswish epilogue; sSE logits and pooled partial sums ride along) ->
//   scse_gates -> [pwconv: skip projection] -> pwconv (scSE gate applied while staging, residual in the epilogue)
//
// dt_pwconv_affine: GEMM M = B*H*W pixels, K = Cin, N = Cout on v_mfma_f32_16x16x4_f32, computed transposed
//   (D^T = W^T A^T) so that a lane ends with 4 consecutive output channels of one pixel: one 16-byte store.
//   A workgroup (4 waves) owns 64 pixels x up to 256 output channels; a wave 16 pixels x all of them.  K runs in chunks
//   of 16 through LDS (register prefetch of the next chunk under the MFMAs of the current one).  The A operand is the
//   virtual input of the other convolution kernels: src0 (optionally nearest x2 up-sampled) | src1 along channels.
//   Every output element is one fixed-order sum over k: the result of a pixel does not depend on the batch around it.
// dt_dwconv3x3_affine: lanes = (pixel, channel quad); a workgroup owns 256 consecutive pixels of ONE image and all
//   channels; neighbours come through the caches.  Per workgroup one row of channel sums (fixed-order, no atomics).
// dt_scse_gates: one workgroup per image: rows -> mean (fixed order) -> two tiny matrix-vector products.
#include "common.h"

#define PW_TM 64        // pixels per workgroup
#define PW_CK 16        // k per chunk
#define PW_LDA 20       // LDS row stride of the activation chunk [64][16] (+4: conflict-free 16x4 reads, 16-byte rows)
#define PW_MAXNB 16     // 16-channel output tiles per workgroup (256 channels)

#define DW_TP 256       // pixels per workgroup
#define DW_MAXG 6       // channel quads per lane: C <= 4 * 64 * 6 = 1536
#define SC_MAXC 1536

__device__ __forceinline__ float dt_hardswish(float x) {
  const float t = fminf(fmaxf(x + 3.f, 0.f), 6.f);
  return x * t / 6.f;
}
__device__ __forceinline__ float dt_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

struct pw_args {
  const float* src0;
  const float* src1;
  const float* w;       // [K][N]
  float* out;
  const float* scale;
  const float* shift;
  const float* gate_c;  // [B][K] or null
  const float* gate_s;  // [B*H*W] or null
  const float* res;     // [M][N] or null (may alias out)
  long long M;          // B*H*W
  int H, W, Hs, Ws;     // Hs x Ws: stored size of src0
  int C0, C1, K, N, up0, act;
};

static inline int pw_ldb(int nw) {   // row stride of the weight chunk [16][nw]: = 16 (mod 64), or nw itself for one tile
  if (nw == 16) return 16;
  int l = (nw / 64) * 64 + 16;
  while (l < nw) l += 64;
  return l;
}

template <int NB>
__global__ __launch_bounds__(256) void pwconv_affine_kernel(pw_args a, int ldb) {
  __shared__ float lds_a[PW_TM * PW_LDA];
  extern __shared__ float lds_b[];       // [16][ldb]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = lane & 15, kq = lane >> 4;
  const int n0 = blockIdx.y * (PW_MAXNB * 16);
  const int nw = min(a.N - n0, PW_MAXNB * 16);      // output channels of this workgroup (multiple of 16)
  const int nbn = nw >> 4;
  const long long p0 = (long long)blockIdx.x * PW_TM;

  // ---- staging role: pixel sp = tid / 4, channel quad sq = tid % 4 of the chunk
  const int sp = tid >> 2, sq = tid & 3;
  const long long pg = p0 + sp;
  const bool pok = pg < a.M;
  long long row0 = 0, row1 = 0;
  int bimg = 0;
  float sig = 0.f;
  if (pok) {
    const long long hw = (long long)a.H * a.W;
    bimg = (int)(pg / hw);
    const int rem = (int)(pg - (long long)bimg * hw);
    const int y = rem / a.W, x = rem - y * a.W;
    row1 = pg;
    row0 = a.up0 ? ((long long)bimg * a.Hs + (y >> 1)) * a.Ws + (x >> 1) : pg;
    if (a.gate_s != nullptr) sig = dt_sigmoid(a.gate_s[pg]);
  }
  const int nbq = 4 * nw;                           // float4 of a weight chunk
  auto load_a = [&](int k0) -> f32x4 {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (pok) {
      const int k = k0 + 4 * sq;
      v = k < a.C0 ? *reinterpret_cast<const f32x4*>(a.src0 + row0 * a.C0 + k)
                   : *reinterpret_cast<const f32x4*>(a.src1 + row1 * a.C1 + (k - a.C0));
      if (a.gate_c != nullptr) {
        const f32x4 g = *reinterpret_cast<const f32x4*>(a.gate_c + (long long)bimg * a.K + k);
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = v[i] * (g[i] + sig);
      }
    }
    return v;
  };
  auto load_b = [&](int k0, int it) -> f32x4 {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    const int idx = tid + it * 256;
    if (idx < nbq) {
      const int q4 = nw >> 2;
      const int kr = idx / q4, q = idx - kr * q4;
      v = *reinterpret_cast<const f32x4*>(a.w + (long long)(k0 + kr) * a.N + n0 + 4 * q);
    }
    return v;
  };

  f32x4 acc[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};

  constexpr int BIT = (NB * 16 * 4 + 255) / 256;    // float4 per thread of a weight chunk: NB / 4, at least 1
  f32x4 ra = load_a(0);
  f32x4 rb[BIT];
#pragma unroll
  for (int it = 0; it < BIT; ++it) rb[it] = load_b(0, it);

  const int abase = (wave * 16 + m) * PW_LDA + kq;
  for (int k0 = 0; k0 < a.K; k0 += PW_CK) {
    __syncthreads();
    *reinterpret_cast<f32x4*>(lds_a + sp * PW_LDA + 4 * sq) = ra;
#pragma unroll
    for (int it = 0; it < BIT; ++it) {
      const int idx = tid + it * 256;
      if (idx < nbq) {
        const int q4 = nw >> 2;
        const int kr = idx / q4, q = idx - kr * q4;
        *reinterpret_cast<f32x4*>(lds_b + kr * ldb + 4 * q) = rb[it];
      }
    }
    __syncthreads();
    if (k0 + PW_CK < a.K) {
      ra = load_a(k0 + PW_CK);
#pragma unroll
      for (int it = 0; it < BIT; ++it) rb[it] = load_b(k0 + PW_CK, it);
    }
#pragma unroll
    for (int s = 0; s < PW_CK / 4; ++s) {
      const float av = lds_a[abase + 4 * s];                 // activation[pixel m][k = 4 s + kq]: the B operand
      const float* bp = lds_b + (4 * s + kq) * ldb + m;      // weight[k][n = 16 nb + m]: the A operand
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
        if (nb < nbn) acc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(bp[nb * 16], av, acc[nb], 0, 0, 0);
    }
  }
  // ---- epilogue: D column = lane & 15 = pixel, rows 4 (lane >> 4) + reg = 4 consecutive output channels
  const long long po = p0 + wave * 16 + m;
  if (po < a.M) {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      if (nb < nbn) {
        const int n = n0 + nb * 16 + 4 * kq;
        const f32x4 sc = *reinterpret_cast<const f32x4*>(a.scale + n);
        const f32x4 sh = *reinterpret_cast<const f32x4*>(a.shift + n);
        f32x4 v;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float t = acc[nb][i] * sc[i] + sh[i];
          v[i] = a.act ? dt_hardswish(t) : t;
        }
        if (a.res != nullptr) {
          const f32x4 r = *reinterpret_cast<const f32x4*>(a.res + po * a.N + n);
#pragma unroll
          for (int i = 0; i < 4; ++i) v[i] += r[i];
        }
        *reinterpret_cast<f32x4*>(a.out + po * a.N + n) = v;
      }
    }
  }
}

template <int NB>
static void pw_launch(const pw_args& a, hipStream_t st) {
  const int nw = a.N < PW_MAXNB * 16 ? a.N : PW_MAXNB * 16;
  const int ldb = pw_ldb(nw);
  dim3 grid((unsigned)((a.M + PW_TM - 1) / PW_TM), (unsigned)dt_cdiv(a.N, PW_MAXNB * 16));
  hipLaunchKernelGGL(pwconv_affine_kernel<NB>, grid, dim3(256), (size_t)PW_CK * ldb * sizeof(float), st, a, ldb);
}

extern "C" int dt_pwconv_affine(const float* src0, const float* src1, const float* w_io, float* out, const float* scale,
                                const float* shift, const float* gate_c, const float* gate_s, const float* res, int B,
                                int H, int W, int C0, int C1, int up0, int Cout, int act, void* stream) {
  DT_REQUIRE(src0 && w_io && out && scale && shift, "pwconv_affine: null operand");
  DT_REQUIRE(B > 0 && H > 0 && W > 0, "pwconv_affine: bad size B=%d H=%d W=%d", B, H, W);
  DT_REQUIRE(C0 > 0 && C0 % 16 == 0 && C1 >= 0 && C1 % 16 == 0, "pwconv_affine: C0=%d / C1=%d must be multiples of 16",
             C0, C1);
  DT_REQUIRE(Cout > 0 && Cout % 16 == 0, "pwconv_affine: Cout=%d must be a multiple of 16", Cout);
  DT_REQUIRE((C1 == 0) == (src1 == nullptr), "pwconv_affine: src1 and C1 must come together");
  DT_REQUIRE((gate_c == nullptr) == (gate_s == nullptr), "pwconv_affine: the channel and the spatial gate come together");
  DT_REQUIRE(up0 == 0 || up0 == 1, "pwconv_affine: up0=%d must be 0 or 1", up0);
  DT_REQUIRE(act == 0 || act == 1, "pwconv_affine: act=%d must be 0 (none) or 1 (Hardswish)", act);
  const long long M = (long long)B * H * W;
  DT_REQUIRE(M * (C0 + C1) < (1ll << 40) && M / PW_TM < (1ll << 31) - 1, "pwconv_affine: tensor too large");
  pw_args a;
  a.src0 = src0, a.src1 = src1, a.w = w_io, a.out = out, a.scale = scale, a.shift = shift;
  a.gate_c = gate_c, a.gate_s = gate_s, a.res = res;
  a.M = M, a.H = H, a.W = W, a.Hs = up0 ? (H + 1) / 2 : H, a.Ws = up0 ? (W + 1) / 2 : W;
  a.C0 = C0, a.C1 = C1, a.K = C0 + C1, a.N = Cout, a.up0 = up0, a.act = act;
  const hipStream_t st = (hipStream_t)stream;
  const int nb = (Cout < PW_MAXNB * 16 ? Cout : PW_MAXNB * 16) / 16;
  if (nb <= 1) pw_launch<1>(a, st);
  else if (nb <= 2) pw_launch<2>(a, st);
  else if (nb <= 4) pw_launch<4>(a, st);
  else if (nb <= 8) pw_launch<8>(a, st);
  else pw_launch<16>(a, st);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

// ------------------------------------------------------------------ depthwise 3x3 + BN + Hardswish (+ sSE logits, pooled sums)
// LQ lanes (a power of two, 4 .. 64) share a pixel: lane ql of them owns the channel quads ql, ql + LQ, ... (at most GT)
template <int LQ, int GT>
__global__ __launch_bounds__(256) void dwconv3x3_affine_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                               const float* __restrict__ scale,
                                                               const float* __restrict__ shift,
                                                               const float* __restrict__ ws, const float* __restrict__ bs,
                                                               float* __restrict__ out, float* __restrict__ s,
                                                               float* __restrict__ part, int H, int W, int C, int P) {
  constexpr int PS = 256 / LQ;                      // pixels per pass
  extern __shared__ float red[];                    // [PS][G * LQ * 4]
  const int tid = threadIdx.x;
  const int ql = tid % LQ, slot = tid / LQ;
  const int CQ = C >> 2, G = (CQ + LQ - 1) / LQ, CP = G * LQ * 4;
  const int b = blockIdx.y, tile = blockIdx.x;
  const int HW = H * W;
  const float* xb = x + (size_t)b * HW * C;
  f32x4 sum[GT];
#pragma unroll
  for (int g = 0; g < GT; ++g) sum[g] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int pass = 0; pass < DW_TP / PS; ++pass) {
    const int p = tile * DW_TP + pass * PS + slot;  // uniform over the LQ lanes of a pixel
    if (p >= HW) break;                             // later passes are further out still
    const int y = p / W, xx = p - y * W;
    float sdot = 0.f;
#pragma unroll
    for (int g = 0; g < GT; ++g) {
      const int cq = ql + g * LQ;
      if (g < G && cq < CQ) {
        const int c = 4 * cq;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
          const int iy = y + kh - 1;
#pragma unroll
          for (int kw = 0; kw < 3; ++kw) {
            const int ix = xx + kw - 1;
            if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) {
              const f32x4 v = *reinterpret_cast<const f32x4*>(xb + ((size_t)iy * W + ix) * C + c);
              const f32x4 k = *reinterpret_cast<const f32x4*>(w + (kh * 3 + kw) * C + c);
#pragma unroll
              for (int i = 0; i < 4; ++i) acc[i] += v[i] * k[i];
            }
          }
        }
        const f32x4 sc = *reinterpret_cast<const f32x4*>(scale + c);
        const f32x4 sh = *reinterpret_cast<const f32x4*>(shift + c);
        const f32x4 wv = *reinterpret_cast<const f32x4*>(ws + c);
        f32x4 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          o[i] = dt_hardswish(acc[i] * sc[i] + sh[i]);
          sum[g][i] += o[i];
          sdot += o[i] * wv[i];
        }
        *reinterpret_cast<f32x4*>(out + ((size_t)b * HW + p) * C + c) = o;
      }
    }
    // the pixel's sSE logit: butterfly over its LQ lanes (fixed order)
#pragma unroll
    for (int o = LQ >> 1; o > 0; o >>= 1) sdot += __shfl_xor(sdot, o, 64);
    if (ql == 0) s[(size_t)b * HW + p] = sdot + bs[0];
  }
  // ---- channel sums of this workgroup's pixels: slots in ascending order
#pragma unroll
  for (int g = 0; g < GT; ++g)
    if (g < G) *reinterpret_cast<f32x4*>(red + slot * CP + 4 * (ql + g * LQ)) = sum[g];
  __syncthreads();
  for (int cq = tid; cq < CQ; cq += 256) {
    f32x4 t = *reinterpret_cast<const f32x4*>(red + 4 * cq);
    for (int sl = 1; sl < PS; ++sl) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(red + sl * CP + 4 * cq);
#pragma unroll
      for (int i = 0; i < 4; ++i) t[i] += v[i];
    }
    *reinterpret_cast<f32x4*>(part + ((size_t)b * P + tile) * C + 4 * cq) = t;
  }
}

extern "C" int dt_dwconv3x3_rows(int H, int W) {
  if (H <= 0 || W <= 0 || (long long)H * W > (1ll << 30)) {
    dt_set_error("dwconv3x3_rows: bad size H=%d W=%d", H, W);
    return DT_EINVAL;
  }
  return dt_cdiv((long long)H * W, DW_TP);
}

static int dw_lq(int C) {
  const int cq = C / 4;
  int lq = 4;
  while (lq * 2 <= cq && lq < 64) lq *= 2;
  return lq;
}

extern "C" int dt_dwconv3x3_affine(const float* x, const float* w_tc, const float* scale, const float* shift,
                                   const float* sse_w, const float* sse_b, float* out, float* s, float* part, int B, int H,
                                   int W, int C, void* stream) {
  DT_REQUIRE(x && w_tc && scale && shift && sse_w && sse_b && out && s && part, "dwconv3x3_affine: null operand");
  DT_REQUIRE(B > 0 && B < 65536 && H > 0 && W > 0 && (long long)H * W <= (1ll << 30),
             "dwconv3x3_affine: bad size B=%d H=%d W=%d", B, H, W);
  DT_REQUIRE(C >= 16 && C % 16 == 0 && C <= 4 * 64 * DW_MAXG, "dwconv3x3_affine: C=%d must be a multiple of 16 in [16, %d]", C,
             4 * 64 * DW_MAXG);
  DT_REQUIRE(x != out, "dwconv3x3_affine: in-place not supported (neighbouring pixels are read)");
  const int P = dt_cdiv((long long)H * W, DW_TP);
  const int lq = dw_lq(C);
  const int G = (C / 4 + lq - 1) / lq;
  const size_t lds = (size_t)(256 / lq) * G * lq * 4 * sizeof(float);
  const dim3 grid(P, B);
  const hipStream_t st = (hipStream_t)stream;
#define DW_GO(LQ_, GT_)                                                                                             \
  hipLaunchKernelGGL((dwconv3x3_affine_kernel<LQ_, GT_>), grid, dim3(256), lds, st, x, w_tc, scale, shift, sse_w, sse_b, \
                     out, s, part, H, W, C, P)
  if (lq == 4) DW_GO(4, 1);
  else if (lq == 8) DW_GO(8, 2);         // C = 48: 12 quads on 8 lanes
  else if (lq == 16) DW_GO(16, 2);
  else if (lq == 32) DW_GO(32, 2);
  else if (G == 1) DW_GO(64, 1);
  else if (G == 2) DW_GO(64, 2);
  else if (G == 3) DW_GO(64, 3);
  else if (G == 4) DW_GO(64, 4);
  else DW_GO(64, DW_MAXG);
#undef DW_GO
  DT_LAUNCH_CHECK();
  return DT_OK;
}

// ------------------------------------------------------------------ scSE channel gate: gc = sigmoid(W2 relu(W1 mean + b1) + b2)
__global__ __launch_bounds__(256) void scse_gates_kernel(const float* __restrict__ part, const float* __restrict__ w1,
                                                         const float* __restrict__ b1, const float* __restrict__ w2,
                                                         const float* __restrict__ b2, float* __restrict__ gc, int P,
                                                         int C, int Ch, float inv_hw, int S) {
  __shared__ float mean[SC_MAXC];
  __shared__ float hid[SC_MAXC];
  extern __shared__ float sl[];                     // [S][C] slice sums (S > 1)
  const int tid = threadIdx.x, b = blockIdx.x;
  const float* pb = part + (size_t)b * P * C;
  if (S == 1) {
    for (int c = tid; c < C; c += 256) {
      float t = 0.f;
      for (int r = 0; r < P; ++r) t += pb[(size_t)r * C + c];
      mean[c] = t * inv_hw;
    }
  } else {
    // slice sl_ of the rows (a contiguous range, the same for every image), then the slices in ascending order
    const int c = tid % C, si = tid / C;
    const int per = (P + S - 1) / S;
    if (si < S) {
      float t = 0.f;
      const int r1 = min(P, (si + 1) * per);
      for (int r = si * per; r < r1; ++r) t += pb[(size_t)r * C + c];
      sl[si * C + c] = t;
    }
    __syncthreads();
    if (tid < C) {
      float t = sl[tid];
      for (int k = 1; k < S; ++k) t += sl[k * C + tid];
      mean[tid] = t * inv_hw;
    }
  }
  __syncthreads();
  for (int j = tid; j < Ch; j += 256) {
    float t = b1[j];
    for (int c = 0; c < C; ++c) t += w1[(size_t)c * Ch + j] * mean[c];
    hid[j] = t > 0.f ? t : 0.f;
  }
  __syncthreads();
  for (int c = tid; c < C; c += 256) {
    float t = b2[c];
    for (int j = 0; j < Ch; ++j) t += w2[(size_t)j * C + c] * hid[j];
    gc[(size_t)b * C + c] = dt_sigmoid(t);
  }
}

extern "C" int dt_scse_gates(const float* part, const float* w1_io, const float* b1, const float* w2_io, const float* b2,
                             float* gc, int B, int P, int C, int Ch, int HW, void* stream) {
  DT_REQUIRE(part && w1_io && b1 && w2_io && b2 && gc, "scse_gates: null operand");
  DT_REQUIRE(B > 0 && P > 0 && HW > 0, "scse_gates: bad size B=%d P=%d HW=%d", B, P, HW);
  DT_REQUIRE(C > 0 && C % 4 == 0 && C <= SC_MAXC, "scse_gates: C=%d must be a multiple of 4 up to %d", C, SC_MAXC);
  DT_REQUIRE(Ch > 0 && Ch <= C, "scse_gates: hidden width %d must lie in [1, C=%d]", Ch, C);
  int S = 1;
  while (2 * S * C <= 256 && 2 * S <= P) S *= 2;
  hipLaunchKernelGGL(scse_gates_kernel, dim3(B), dim3(256), S > 1 ? (size_t)S * C * sizeof(float) : 0, (hipStream_t)stream,
                     part, w1_io, b1, w2_io, b2, gc, P, C, Ch, 1.f / (float)HW, S);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

// ------------------------------------------------------------------ eval BatchNorm behind a biased convolution
// BN(conv + bias) = conv * scale + (beta - mean * scale + scale * bias): dt_bn_eval_affine with the bias folded in
__global__ void bn_eval_affine_bias_kernel(const float* gamma, const float* beta, const float* rm, const float* rv,
                                           const float* bias, float eps, int C, float* scale, float* shift) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < C) {
    const float is = 1.f / sqrtf(rv[c] + eps);
    const float sc = gamma[c] * is;
    scale[c] = sc;
    shift[c] = (beta[c] - rm[c] * sc) + sc * bias[c];
  }
}

extern "C" int dt_bn_eval_affine_bias(const float* gamma, const float* beta, const float* rm, const float* rv,
                                      const float* bias, float eps, int C, float* scale, float* shift, void* stream) {
  DT_REQUIRE(gamma && beta && rm && rv && bias && scale && shift && C > 0, "bn_eval_affine_bias: bad args");
  hipLaunchKernelGGL(bn_eval_affine_bias_kernel, dim3(dt_cdiv(C, 256)), dim3(256), 0, (hipStream_t)stream, gamma, beta,
                     rm, rv, bias, eps, C, scale, shift);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

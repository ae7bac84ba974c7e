// MDL-RS fusion CNNs (model/compare_method/DML_Hong.py: Early / Middle / Late / Cross_fusion_CNN; DESIGN.md
// section 19): the ops no other model has.
//   vc_maxpool2p_fwd / _bwd        MaxPool2d(kernel 2, stride 2, padding 1) with the preceding BatchNorm + ReLU folded in
//   vc_avgpool_head_fwd / _bwd     AdaptiveAvgPool2d(1) + conv7 (1x1 on a 1x1 map = a product) for 1..3 maps
//   vc_xfusion_loss_fwd_bwd        Cross_fusion_CNN_Loss (losses.py:7-19) and its three logit gradients
// All fp32; every sum runs in a fixed order (no atomics), so results are run-to-run identical.
#include "common.h"

namespace {

// norm.hip's bn_fwd_elem, the BatchNorm forward's own arithmetic: the fused pool sees the bits vc_bn_apply writes
__device__ __forceinline__ float pool_bn_elem(float xv, float mean, float invstd, float w, float b) {
#pragma clang fp contract(off)
  return fmaf((xv - mean) * invstd, w, b);
}

// ---------------------------------------------------------------- padded 2x2 / stride 2 max pool
// Output (oh, ow) covers input rows 2 oh - 1, 2 oh and columns 2 ow - 1, 2 ow; taps outside the map are -inf
// padding and never win.  arg = kh * 2 + kw of the first maximum among the in-range taps in (kh, kw) order, as torch
// (NaN propagates).  With bn_*: each tap is relu((x - mean) * invstd * w + b) first.
__global__ void maxpool2p(int total, FastDiv fC, FastDiv fOW, FastDiv fOH, int H, int W, const float* __restrict__ x,
                          long ldx, const float* __restrict__ mean, const float* __restrict__ invstd,
                          const float* __restrict__ bw, const float* __restrict__ bb, float* __restrict__ y,
                          unsigned char* __restrict__ arg) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  int c, ow, oh;
  const int q = fdivmod(idx, fC, c);
  const int r = fdivmod(q, fOW, ow);
  const int bb_ = fdivmod(r, fOH, oh);
  float m = 0.f, is = 0.f, gw = 0.f, gb = 0.f;
  if (mean) {
    m = mean[c];
    is = invstd[c];
    gw = bw[c];
    gb = bb[c];
  }
  float best = -INFINITY;
  int bi = -1;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int ih = 2 * oh - 1 + (t >> 1), iw = 2 * ow - 1 + (t & 1);
    if (ih < 0 || ih >= H || iw < 0 || iw >= W) continue;
    float v = x[(((long)bb_ * H + ih) * W + iw) * ldx + c];
    if (mean) v = fmaxf(pool_bn_elem(v, m, is, gw, gb), 0.f);
    if (bi < 0 || v > best || isnan(v)) {
      best = v;
      bi = t;
    }
  }
  y[idx] = best;
  arg[idx] = (unsigned char)bi;
}

// gather form of the backward: input pixel (h, w) belongs to window ((h + 1) / 2, (w + 1) / 2) as tap
// ((h + 1) & 1, (w + 1) & 1) and to no other (stride = kernel), so every dx element is written exactly once
__global__ void maxpool2p_bwd(int total, FastDiv fC, FastDiv fW, FastDiv fH, const float* __restrict__ dy,
                              const unsigned char* __restrict__ arg, const float* __restrict__ y,
                              float* __restrict__ dx, long lddx) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int C = fC.div, H = fH.div, W = fW.div;
  const int OH = H / 2 + 1, OW = W / 2 + 1;
  int c, iw, ih;
  const int p = fdivmod(idx, fC, c);
  const int q = fdivmod(p, fW, iw);
  const int b = fdivmod(q, fH, ih);
  const int oh = (ih + 1) >> 1, ow = (iw + 1) >> 1;
  const int t = (((ih + 1) & 1) << 1) | ((iw + 1) & 1);
  const int o = ((b * OH + oh) * OW + ow) * C + c;
  float v = 0.f;
  if (arg[o] == t && (!y || y[o] > 0.f)) v = dy[o];
  dx[(long)p * lddx + c] = v;
}

// ---------------------------------------------------------------- average-pool head
// Rows r of the classifier's operand: concat mode (0): r = b, column j = g * C + c (cat[x1, x2] of the late model);
// separate mode (1): r = g * B + b, column j = c (the cross model's three heads, one shared weight).
struct HeadMaps {
  const float* f[3];
};
struct HeadGrads {
  float* d[3];
};

// block per row: pooled[r, j] = mean_p f_g[b, p, c] (pixels summed in order by one thread), then
// logits[r, k] = sum_j pooled[r, j] W[k, j] + bias[k] (a 16-lane row per class, DPP row sums)
__global__ __launch_bounds__(256) void avgpool_head_fwd(int B, int HW, int C, int Cin, int ncls, int mode, HeadMaps maps,
                                                        const float* __restrict__ W, const float* __restrict__ bias,
                                                        float* __restrict__ pooled, float* __restrict__ logits) {
  extern __shared__ float fs[];   // [Cin]
  const int r = blockIdx.x;
  const float inv = 1.f / (float)HW;
  for (int j = threadIdx.x; j < Cin; j += 256) {
    const int g = mode ? r / B : j / C, b = mode ? r % B : r, c = mode ? j : j % C;
    const float* f = maps.f[g] + (long)b * HW * C + c;
    float s = 0.f;
    for (int p = 0; p < HW; ++p) s += f[(long)p * C];
    s *= inv;
    fs[j] = s;
    pooled[(long)r * Cin + j] = s;
  }
  __syncthreads();
  const int gl = threadIdx.x >> 4, l = threadIdx.x & 15;
  for (int k0 = 0; k0 < ncls; k0 += 16) {
    const int k = k0 + gl;
    float acc = 0.f;
    if (k < ncls)
      for (int j = l; j < Cin; j += 16) acc += fs[j] * W[(long)k * Cin + j];
    acc = row16_sum(acc);
    if (l == 0 && k < ncls) logits[(long)r * ncls + k] = acc + bias[k];
  }
}

// blocks [0, R): the map gradient of row r, dpooled[r, j] / HW broadcast over the pixels; the rest: tile (k, y) of the
// weight / bias gradient, 64 columns x 4 row groups over the R rows (all applications), fixed-order LDS combine;
// column Cin is the bias gradient
__global__ __launch_bounds__(256) void avgpool_head_bwd(int R, int B, int HW, int C, int Cin, int ncls, int mode,
                                                        const float* __restrict__ dlog, const float* __restrict__ W,
                                                        const float* __restrict__ pooled, HeadGrads df,
                                                        float* __restrict__ dW, float* __restrict__ db) {
  const int bid = blockIdx.x;
  if (bid < R) {
    const int r = bid;
    const float inv = 1.f / (float)HW;
    for (int j = threadIdx.x; j < Cin; j += 256) {
      float gsum = 0.f;
      for (int k = 0; k < ncls; ++k) gsum += dlog[(long)r * ncls + k] * W[(long)k * Cin + j];
      gsum *= inv;
      const int g = mode ? r / B : j / C, b = mode ? r % B : r, c = mode ? j : j % C;
      float* d = df.d[g] + (long)b * HW * C + c;
      for (int p = 0; p < HW; ++p) d[(long)p * C] = gsum;
    }
    return;
  }
  __shared__ float red[4][64];
  const int t = bid - R;
  const int k = t % ncls, yy = t / ncls;
  const int cl = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const int j = yy * 64 + cl;
  float acc = 0.f;
  if (j <= Cin)
    for (int r = rg; r < R; r += 4) acc += dlog[(long)r * ncls + k] * (j < Cin ? pooled[(long)r * Cin + j] : 1.f);
  red[rg][cl] = acc;
  __syncthreads();
  if (rg == 0 && j <= Cin) {
    const float v = red[0][cl] + red[1][cl] + red[2][cl] + red[3][cl];
    if (j < Cin) dW[(long)k * Cin + j] = v;
    else db[k] = v;
  }
}

// ---------------------------------------------------------------- cross-fusion loss
// One 1024-thread block.  The cross-entropy half is misc.hip's ce_fwd_bwd code (a 16-lane row per sample), so with
// o2 = o3 = o1 the loss and do1 carry vc_ce_fwd_bwd's bits.
constexpr int XLT = 1024;

__device__ __forceinline__ float xl_row16_max(float v) {
  v = fmaxf(v, dpp_mov<0xB1>(v));
  v = fmaxf(v, dpp_mov<0x4E>(v));
  v = fmaxf(v, dpp_mov<0x141>(v));
  v = fmaxf(v, dpp_mov<0x140>(v));
  return v;
}

__device__ __forceinline__ void xl_ce_row(const float* __restrict__ lr, int ncls, long long y, int l, float& mx,
                                          float& se, float& ly) {
  mx = -INFINITY;
  float t = 0.f;
  for (int k = l; k < ncls; k += 16) {
    const float v = lr[k];
    mx = fmaxf(mx, v);
    if (k == y) t = v;
  }
  mx = xl_row16_max(mx);
  ly = row16_sum(t);
  se = 0.f;
  for (int k = l; k < ncls; k += 16) se += __expf(lr[k] - mx);
  se = row16_sum(se);
}

__device__ __forceinline__ float xl_block_sum(float v, float* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = 0.f;
#pragma unroll
  for (int i = 0; i < XLT / 64; ++i) r += red[i];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(XLT) void xfusion_loss(int B, int ncls, const float* __restrict__ o1,
                                                    const float* __restrict__ o2, const float* __restrict__ o3,
                                                    const long long* __restrict__ target, const float* __restrict__ w,
                                                    float* __restrict__ loss, float* __restrict__ do1,
                                                    float* __restrict__ do2, float* __restrict__ do3) {
  __shared__ float red[XLT / 64];
  const long long ignore_index = -100;   // nn.CrossEntropyLoss's default, as the reference constructs it
  const int g = threadIdx.x >> 4, l = threadIdx.x & 15;
  // weighted mean cross entropy of o1
  float num = 0.f, den = 0.f;
  for (int b = g; b < B; b += XLT / 16) {
    const long long y = target[b];
    float mx, se, ly;
    xl_ce_row(o1 + (long)b * ncls, ncls, y, l, mx, se, ly);
    if (l == 0 && y != ignore_index) {
      const float wy = w ? w[y] : 1.f;
      num += wy * (logf(se) + mx - ly);
      den += wy;
    }
  }
  num = xl_block_sum(num, red);
  den = xl_block_sum(den, red);
  // the two mean squared differences over all B * ncls elements
  const int n = B * ncls;
  float s2 = 0.f, s3 = 0.f;
  for (int i = threadIdx.x; i < n; i += XLT) {
    const float a = o1[i], d2 = a - o2[i], d3 = a - o3[i];
    s2 += d2 * d2;
    s3 += d3 * d3;
  }
  s2 = xl_block_sum(s2, red);
  s3 = xl_block_sum(s3, red);
  const float invn = 1.f / (float)n;
  if (threadIdx.x == 0) loss[0] = num / den + s2 * invn + s3 * invn;
  // gradients for d(loss) = 1
  float dsum = 0.f;
  for (int b = threadIdx.x; b < B; b += XLT) {
    const long long y = target[b];
    if (y != ignore_index) dsum += w ? w[y] : 1.f;
  }
  dsum = xl_block_sum(dsum, red);
  const float gs = 1.f / dsum;
  const float c2 = 2.f * invn;
  for (int b = g; b < B; b += XLT / 16) {
    const long long y = target[b];
    float mx, se, ly;
    const float* lr = o1 + (long)b * ncls;
    xl_ce_row(lr, ncls, y, l, mx, se, ly);
    const float wy = (y == ignore_index) ? 0.f : (w ? w[y] : 1.f);
    for (int k = l; k < ncls; k += 16) {
      const long i = (long)b * ncls + k;
      const float p = __expf(lr[k] - mx) / se;
      const float ce = gs * wy * (p - (k == y ? 1.f : 0.f));
      const float g2 = c2 * (lr[k] - o2[i]), g3 = c2 * (lr[k] - o3[i]);
      do1[i] = ce + g2 + g3;
      do2[i] = -g2;
      do3[i] = -g3;
    }
  }
}

}  // namespace

VC_API int vc_maxpool2p_fwd(int B, int H, int W, int C, const float* x, long ldx, const float* bn_mean,
                            const float* bn_invstd, const float* bn_w, const float* bn_b, float* y, unsigned char* arg,
                            hipStream_t stream) {
  VC_REQUIRE(B >= 0 && H >= 2 && W >= 2 && C > 0 && ldx >= C);
  const int nbn = (bn_mean != nullptr) + (bn_invstd != nullptr) + (bn_w != nullptr) + (bn_b != nullptr);
  VC_REQUIRE(nbn == 0 || nbn == 4);
  const int OH = H / 2 + 1, OW = W / 2 + 1;
  const long total = (long)B * OH * OW * C;
  if (total == 0) return VC_OK;
  VC_REQUIRE(x && y && arg);
  VC_REQUIRE_I32(total);
  VC_REQUIRE_I32((long)B * H * W * ldx);
  hipLaunchKernelGGL(maxpool2p, dim3(vc_cdiv(total, 256)), dim3(256), 0, stream, (int)total, make_fastdiv(C),
                     make_fastdiv(OW), make_fastdiv(OH), H, W, x, ldx, bn_mean, bn_invstd, bn_w, bn_b, y, arg);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

VC_API int vc_maxpool2p_bwd(int B, int H, int W, int C, const float* dy, const unsigned char* arg, const float* y,
                            float* dx, long lddx, hipStream_t stream) {
  VC_REQUIRE(B >= 0 && H >= 2 && W >= 2 && C > 0 && lddx >= C);
  const long total = (long)B * H * W * C;
  if (total == 0) return VC_OK;
  VC_REQUIRE(dy && arg && dx);
  VC_REQUIRE_I32((long)B * H * W * lddx);
  VC_REQUIRE_I32((long)B * (H / 2 + 1) * (W / 2 + 1) * C);
  hipLaunchKernelGGL(maxpool2p_bwd, dim3(vc_cdiv(total, 256)), dim3(256), 0, stream, (int)total, make_fastdiv(C),
                     make_fastdiv(W), make_fastdiv(H), dy, arg, y, dx, lddx);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

static bool head_ok(int B, int HW, int C, int G, int ncls, int mode) {
  return B > 0 && HW > 0 && C > 0 && C <= 1024 && G >= 1 && G <= 3 && ncls > 0 && (mode == 0 || mode == 1) &&
         (long)G * B * HW * C < (1L << 31) && (long)G * B * ncls < (1L << 31);
}

VC_API int vc_avgpool_head_fwd(int B, int HW, int C, int G, int ncls, int mode, const float* f0, const float* f1,
                               const float* f2, const float* W, const float* bias, float* pooled, float* logits,
                               hipStream_t stream) {
  VC_REQUIRE(head_ok(B, HW, C, G, ncls, mode));
  VC_REQUIRE(f0 && (G < 2 || f1) && (G < 3 || f2) && W && bias && pooled && logits);
  const int R = mode ? G * B : B, Cin = mode ? C : G * C;
  HeadMaps maps{{f0, f1, f2}};
  hipLaunchKernelGGL(avgpool_head_fwd, dim3(R), dim3(256), sizeof(float) * Cin, stream, B, HW, C, Cin, ncls, mode, maps,
                     W, bias, pooled, logits);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

VC_API int vc_avgpool_head_bwd(int B, int HW, int C, int G, int ncls, int mode, const float* dlogits, const float* W,
                               const float* pooled, float* df0, float* df1, float* df2, float* dW, float* db,
                               hipStream_t stream) {
  VC_REQUIRE(head_ok(B, HW, C, G, ncls, mode));
  VC_REQUIRE(dlogits && W && pooled && df0 && (G < 2 || df1) && (G < 3 || df2) && dW && db);
  const int R = mode ? G * B : B, Cin = mode ? C : G * C;
  HeadGrads df{{df0, df1, df2}};
  hipLaunchKernelGGL(avgpool_head_bwd, dim3(R + ncls * vc_cdiv(Cin + 1, 64)), dim3(256), 0, stream, R, B, HW, C, Cin,
                     ncls, mode, dlogits, W, pooled, df, dW, db);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

VC_API int vc_xfusion_loss_fwd_bwd(int B, int ncls, const float* o1, const float* o2, const float* o3,
                                   const long long* target, const float* weight, float* loss, float* do1, float* do2,
                                   float* do3, hipStream_t stream) {
  VC_REQUIRE(B > 0 && ncls > 0 && (long)B * ncls < (1L << 31));
  VC_REQUIRE(o1 && o2 && o3 && target && loss && do1 && do2 && do3);
  hipLaunchKernelGGL(xfusion_loss, dim3(1), dim3(XLT), 0, stream, B, ncls, o1, o2, o3, target, weight, loss, do1, do2,
                     do3);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

// Per-pixel comparison models (model/compare_method/EndNet.py, spectralformer.py): the ops no
// other model has.
//   vc_fc_fused_fwd / _bwd         Linear + {BatchNorm1d + ReLU | sigmoid | nothing}, column-owned: ONE launch per layer
//   vc_endnet_loss_fwd_bwd         EndNet_Loss (losses.py:21-35) and its three gradients
//   vc_sf_embed_fwd / _bwd         SpectralFormer's Linear(1, dim) embedding + cls row + position (+ dropout)
// All fp32, plain FMA (the layers are latency-bound: K <= 512, a few hundred rows), no atomics; every sum runs in a
// fixed order, so a second call repeats its bits.
#include "common.h"

namespace {

// ---------------------------------------------------------------- fused fully-connected layer
// A workgroup owns FC_NC output columns.  LDS plan (static, 49.3 KiB of the CU's 160 KiB: three workgroups per CU):
//   ws  [FC_NC][FC_KMAX + 1]   the columns' weight rows (odd row stride: the 8 columns of a wave hit 8 banks)  16.0 KiB
//   zs  [FC_BMAX][FC_NC]       x W^T + b of every batch row (train-mode BatchNorm only)                       32.0 KiB
//   red [32][FC_NC], st        per-row-group partial sums and the column statistics                            1.1 KiB
// Thread t works on column t & 7 and rows (t >> 3) + 32 i.
constexpr int FC_NC = 8;
constexpr int FC_BMAX = VC_FC_TRAIN_BMAX;
constexpr int FC_KMAX = VC_FC_KMAX;
constexpr int FC_RT = 128;   // rows per workgroup on the row-tiled grid (everything but train-mode BatchNorm)

// x . w over K terms: eight interleaved partial sums combined pairwise (a fixed order).  Against one running sum this
// cuts the dependent FMA chain by 8 and the rounding error's growth with K likewise -- a train-mode BatchNorm column
// whose batch variance is near eps amplifies that error by 1 / sqrt(var + eps).
__device__ __forceinline__ float fc_dot(const float* __restrict__ xr, const float* wr, int K) {
  float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const int K8 = K & ~7;
  for (int k = 0; k < K8; k += 8) {
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = fmaf(xr[k + j], wr[k + j], a[j]);
  }
#pragma unroll
  for (int j = 0; j < 7; ++j)
    if (K8 + j < K) a[j] = fmaf(xr[K8 + j], wr[K8 + j], a[j]);
  return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
}

// sum over the 32 row groups of red[.][c], in order, by threads 0..7; the result to every thread through out[c]
template <typename T>
__device__ __forceinline__ void fc_combine(T (*red)[FC_NC], T* out, T scale) {
  __syncthreads();
  if (threadIdx.x < FC_NC) {
    T s = 0;
#pragma unroll
    for (int j = 0; j < 32; ++j) s += red[j][threadIdx.x];
    out[threadIdx.x] = s * scale;
  }
  __syncthreads();
}

__global__ __launch_bounds__(256) void fc_fused_fwd(int mode, int train, int B, int K, int N, int RT,
                                                    const float* __restrict__ x, long ldx, const float* __restrict__ W,
                                                    const float* __restrict__ bias, const float* __restrict__ gamma,
                                                    const float* __restrict__ beta, float* __restrict__ rmean,
                                                    float* __restrict__ rvar, float eps, float mom, float* __restrict__ y,
                                                    long ldy, float* __restrict__ xhat, float* __restrict__ save_mean,
                                                    float* __restrict__ save_rstd) {
  __shared__ float ws[FC_NC][FC_KMAX + 1];
  __shared__ float zs[FC_BMAX * FC_NC];
  __shared__ float red[32][FC_NC];
  __shared__ float st[2][FC_NC];
  const int tid = threadIdx.x;
  const int n0 = blockIdx.x * FC_NC;
  const int nc = min(FC_NC, N - n0);
  const int r0 = blockIdx.y * RT, r1 = min(B, r0 + RT);
  for (int i = tid; i < nc * K; i += 256) {
    const int c = i / K, k = i - c * K;
    ws[c][k] = W[(long)(n0 + c) * K + k];
  }
  __syncthreads();
  const int c = tid & (FC_NC - 1), rl = tid >> 3;
  const bool live = c < nc;
  const int n = n0 + c;
  const bool bnt = mode == VC_FC_BN_RELU && train;   // uniform over the grid
  const float bv = live ? bias[n] : 0.f;
  float g = 1.f, bt = 0.f, m = 0.f, rs = 1.f;
  if (mode == VC_FC_BN_RELU && live) {
    g = gamma[n];
    bt = beta[n];
    if (!train) {
      m = rmean[n];
      rs = 1.0f / sqrtf(rvar[n] + eps);
      if (blockIdx.y == 0 && rl == 0 && save_mean) {
        save_mean[n] = m;
        save_rstd[n] = rs;
      }
    }
  }
  if (live) {
    for (int r = r0 + rl; r < r1; r += 32) {
      const float z = fc_dot(x + (long)r * ldx, ws[c], K) + bv;
      if (bnt) {
        zs[r * FC_NC + c] = z;   // r0 = 0: one workgroup sees every row
      } else if (mode == VC_FC_BN_RELU) {
        const float xh = (z - m) * rs;
        if (xhat) xhat[(long)r * N + n] = xh;
        y[(long)r * ldy + n] = fmaxf(fmaf(xh, g, bt), 0.f);
      } else if (mode == VC_FC_SIGMOID) {
        y[(long)r * ldy + n] = 1.0f / (1.0f + expf(-z));
      } else {
        y[(long)r * ldy + n] = z;
      }
    }
  }
  if (!bnt) return;
  // batch statistics of the workgroup's columns, two passes over the LDS copy
  __syncthreads();
  float s = 0.f;
  if (live)
    for (int r = rl; r < B; r += 32) s += zs[r * FC_NC + c];
  red[rl][c] = s;
  fc_combine(red, st[0], 1.0f / (float)B);
  const float mean = st[0][c];
  s = 0.f;
  if (live)
    for (int r = rl; r < B; r += 32) {
      const float d = zs[r * FC_NC + c] - mean;
      s = fmaf(d, d, s);
    }
  red[rl][c] = s;
  fc_combine(red, st[1], 1.0f / (float)B);
  const float var = st[1][c];
  const float rstd = 1.0f / sqrtf(var + eps);
  if (live && rl == 0) {
    save_mean[n] = mean;
    save_rstd[n] = rstd;
    rmean[n] = (1.f - mom) * rmean[n] + mom * mean;
    rvar[n] = (1.f - mom) * rvar[n] + mom * (var * ((float)B / (float)(B - 1)));
  }
  if (live)
    for (int r = rl; r < B; r += 32) {
      const float xh = (zs[r * FC_NC + c] - mean) * rstd;
      xhat[(long)r * N + n] = xh;
      y[(long)r * ldy + n] = fmaxf(fmaf(xh, g, bt), 0.f);
    }
}

// the backward of the same columns: the activation's mask, the BatchNorm column sums, dz, then dW / db
__global__ __launch_bounds__(256) void fc_fused_bwd(int mode, int train, int B, int K, int N,
                                                    const float* __restrict__ dy, long lddy, const float* __restrict__ y,
                                                    long ldy, const float* __restrict__ xhat, const float* __restrict__ x,
                                                    long ldx, const float* __restrict__ gamma,
                                                    const float* __restrict__ rstd, float* __restrict__ dz, long lddz,
                                                    float* __restrict__ dW, float* __restrict__ db,
                                                    float* __restrict__ dgamma, float* __restrict__ dbeta) {
  // The column sums, the dz arithmetic and the dW / db accumulation run in fp64 (a few thousand operations per
  // workgroup): a Linear bias in front of a train-mode BatchNorm has a true gradient of 0, and so has the weight at
  // K = 1 -- what is left there is rounding noise, B times the error of the two means in fp32.  dz itself is stored
  // (LDS and global) rounded once to fp32.
  __shared__ float gs[FC_BMAX * FC_NC];
  __shared__ double red[32][FC_NC];
  __shared__ double st[2][FC_NC];
  const int tid = threadIdx.x;
  const int n0 = blockIdx.x * FC_NC;
  const int nc = min(FC_NC, N - n0);
  const int c = tid & (FC_NC - 1), rl = tid >> 3;
  const bool live = c < nc;
  const int n = n0 + c;
  double s1 = 0.0, s2 = 0.0;
  if (live)
    for (int r = rl; r < B; r += 32) {
      float g = dy[(long)r * lddy + n];
      if (mode == VC_FC_BN_RELU) {
        g = y[(long)r * ldy + n] > 0.f ? g : 0.f;
        s1 += (double)g;
        s2 += (double)g * (double)xhat[(long)r * N + n];
      } else if (mode == VC_FC_SIGMOID) {
        const float yv = y[(long)r * ldy + n];
        g *= yv * (1.f - yv);
      }
      gs[r * FC_NC + c] = g;
    }
  double sb = 0.0;   // db = sum_b dz[b, n], of the unrounded dz
  if (mode == VC_FC_BN_RELU) {
    red[rl][c] = s1;
    fc_combine(red, st[0], 1.0);
    red[rl][c] = s2;
    fc_combine(red, st[1], 1.0);
    if (live) {
      const double t1 = st[0][c], t2 = st[1][c];
      if (rl == 0) {
        dbeta[n] = (float)t1;
        dgamma[n] = (float)t2;
      }
      const double sc = (double)gamma[n] * (double)rstd[n], invB = 1.0 / (double)B;
      const double m1 = train ? t1 * invB : 0.0, m2 = train ? t2 * invB : 0.0;
      for (int r = rl; r < B; r += 32) {
        const double v = sc * (((double)gs[r * FC_NC + c] - m1) - (double)xhat[(long)r * N + n] * m2);
        sb += v;
        gs[r * FC_NC + c] = (float)v;
      }
    }
  } else if (live) {
    for (int r = rl; r < B; r += 32) sb += (double)gs[r * FC_NC + c];
  }
  // the dz rows (each thread re-reads only what it wrote: no barrier needed before this loop)
  if (live && dz)
    for (int r = rl; r < B; r += 32) dz[(long)r * lddz + n] = gs[r * FC_NC + c];
  red[rl][c] = sb;
  fc_combine(red, st[0], 1.0);   // its barriers also publish gs to the weight-gradient loop
  if (live && rl == 0) db[n] = (float)st[0][c];
  // dW[n0 + cc, k] = sum_r dz[r, cc] x[r, k]: adjacent threads take adjacent k (coalesced x, broadcast gs); the
  // products of two floats are exact in fp64
  for (int p = tid; p < nc * K; p += 256) {
    const int cc = p / K, k = p - cc * K;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;   // four interleaved partial sums over the rows, a fixed order
    const int B4 = B & ~3;
    const float* xk = x + k;
    for (int r = 0; r < B4; r += 4) {
      a0 += (double)gs[r * FC_NC + cc] * (double)xk[(long)r * ldx];
      a1 += (double)gs[(r + 1) * FC_NC + cc] * (double)xk[(long)(r + 1) * ldx];
      a2 += (double)gs[(r + 2) * FC_NC + cc] * (double)xk[(long)(r + 2) * ldx];
      a3 += (double)gs[(r + 3) * FC_NC + cc] * (double)xk[(long)(r + 3) * ldx];
    }
    for (int r = B4; r < B; ++r) a0 += (double)gs[r * FC_NC + cc] * (double)xk[(long)r * ldx];
    dW[(long)(n0 + cc) * K + k] = (float)((a0 + a1) + (a2 + a3));
  }
}

// ---------------------------------------------------------------- EndNet loss
// One 1024-thread block.  The cross-entropy half is misc.hip's ce_fwd_bwd code (a 16-lane row per sample), as in
// mdlrs.hip's cross-fusion loss: with de = x the loss and dout carry vc_ce_fwd_bwd's bits.
constexpr int ELT = 1024;

__device__ __forceinline__ float el_row16_max(float v) {
  v = fmaxf(v, dpp_mov<0xB1>(v));
  v = fmaxf(v, dpp_mov<0x4E>(v));
  v = fmaxf(v, dpp_mov<0x141>(v));
  v = fmaxf(v, dpp_mov<0x140>(v));
  return v;
}

__device__ __forceinline__ void el_ce_row(const float* __restrict__ lr, int ncls, long long y, int l, float& mx,
                                          float& se, float& ly) {
  mx = -INFINITY;
  float t = 0.f;
  for (int k = l; k < ncls; k += 16) {
    const float v = lr[k];
    mx = fmaxf(mx, v);
    if (k == y) t = v;
  }
  mx = el_row16_max(mx);
  ly = row16_sum(t);
  se = 0.f;
  for (int k = l; k < ncls; k += 16) se += __expf(lr[k] - mx);
  se = row16_sum(se);
}

__device__ __forceinline__ float el_block_sum(float v, float* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = 0.f;
#pragma unroll
  for (int i = 0; i < ELT / 64; ++i) r += red[i];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(ELT) void endnet_loss(int B, int ncls, int C1, int C2, const float* __restrict__ out,
                                                   const long long* __restrict__ target, const float* __restrict__ w,
                                                   const float* __restrict__ de1, const float* __restrict__ x1,
                                                   const float* __restrict__ de2, const float* __restrict__ x2,
                                                   float* __restrict__ loss, float* __restrict__ dout,
                                                   float* __restrict__ dde1, float* __restrict__ dde2) {
  __shared__ float red[ELT / 64];
  const long long ignore_index = -100;   // nn.CrossEntropyLoss's default, as the reference constructs it
  const int g = threadIdx.x >> 4, l = threadIdx.x & 15;
  float num = 0.f, den = 0.f;
  for (int b = g; b < B; b += ELT / 16) {
    const long long y = target[b];
    float mx, se, ly;
    el_ce_row(out + (long)b * ncls, ncls, y, l, mx, se, ly);
    if (l == 0 && y != ignore_index) {
      const float wy = w ? w[y] : 1.f;
      num += wy * (logf(se) + mx - ly);
      den += wy;
    }
  }
  num = el_block_sum(num, red);
  den = el_block_sum(den, red);
  // the two mean squared reconstruction errors, over B C1 and B C2 elements
  const int n1 = B * C1, n2 = B * C2;
  const float c1 = 2.f / (float)n1, c2 = 2.f / (float)n2;
  float s1 = 0.f, s2 = 0.f;
  for (int i = threadIdx.x; i < n1; i += ELT) {
    const float d = de1[i] - x1[i];
    s1 += d * d;
    dde1[i] = c1 * d;
  }
  for (int i = threadIdx.x; i < n2; i += ELT) {
    const float d = de2[i] - x2[i];
    s2 += d * d;
    dde2[i] = c2 * d;
  }
  s1 = el_block_sum(s1, red);
  s2 = el_block_sum(s2, red);
  if (threadIdx.x == 0) loss[0] = num / den + s1 * (1.f / (float)n1) + s2 * (1.f / (float)n2);
  // dout for d(loss) = 1
  float dsum = 0.f;
  for (int b = threadIdx.x; b < B; b += ELT) {
    const long long y = target[b];
    if (y != ignore_index) dsum += w ? w[y] : 1.f;
  }
  dsum = el_block_sum(dsum, red);
  const float gsc = 1.f / dsum;
  for (int b = g; b < B; b += ELT / 16) {
    const long long y = target[b];
    float mx, se, ly;
    const float* lr = out + (long)b * ncls;
    el_ce_row(lr, ncls, y, l, mx, se, ly);
    const float wy = (y == ignore_index) ? 0.f : (w ? w[y] : 1.f);
    for (int k = l; k < ncls; k += 16) {
      const float p = __expf(lr[k] - mx) / se;
      dout[(long)b * ncls + k] = gsc * wy * (p - (k == y ? 1.f : 0.f));
    }
  }
}

// ---------------------------------------------------------------- SpectralFormer embedding
// s2eft.hip's dropout hash (vc_dropout_fwd): keep_i = u_i >= p with u_i = hash(seed, i) / 2^24
__device__ __forceinline__ uint32_t sf_mix32(uint64_t seed, uint32_t i) {
  uint64_t z = seed ^ ((uint64_t)i * 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (uint32_t)((z ^ (z >> 31)) >> 32);
}

__global__ void sf_embed_fwd(int total, FastDiv fD, FastDiv fT, int C1, int C2, const float* __restrict__ x1,
                             const float* __restrict__ x2, const float* __restrict__ w, const float* __restrict__ bias,
                             const float* __restrict__ cls, const float* __restrict__ pos, float p, float scale,
                             unsigned long long seed, const unsigned long long* __restrict__ seed_dev,
                             float* __restrict__ X, unsigned char* __restrict__ mask) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  if (p > 0.f) seed = vc_site_seed(seed, seed_dev);
  int d, t;
  const int q = fdivmod(i, fD, d);
  const int b = fdivmod(q, fT, t);
  const int D = fD.div;
  float v;
  if (t == 0) {
    v = cls[d] + pos[d];
  } else {
    const int nb = t - 1;
    const float xv = nb < C1 ? x1[(long)b * C1 + nb] : x2[(long)b * C2 + (nb - C1)];
    v = fmaf(xv, w[d], bias[d]) + pos[t * D + d];
  }
  if (p > 0.f) {
    const float u = (float)(sf_mix32(seed, (uint32_t)i) >> 8) * (1.0f / 16777216.0f);
    const bool keep = u >= p;
    v = keep ? v * scale : 0.f;
    mask[i] = keep ? 1 : 0;
  }
  X[i] = v;
}

// thread (t, d): the batch sums of dX[., t, d] and of x[., t - 1] dX[., t, d], over b in order
__global__ void sf_embed_bwd_cols(int TD, int D, int B, int C1, int C2, const float* __restrict__ x1,
                                  const float* __restrict__ x2, const float* __restrict__ dX,
                                  const unsigned char* __restrict__ mask, float scale, float* __restrict__ dpos,
                                  float* __restrict__ dcls, float* __restrict__ part) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= TD) return;
  const int t = i / D, d = i - t * D;
  const int nb = t - 1;
  float s = 0.f, sx = 0.f;
  for (int b = 0; b < B; ++b) {
    const long j = (long)b * TD + i;
    float g = dX[j];
    if (mask) g = mask[j] ? g * scale : 0.f;
    s += g;
    if (t > 0) sx = fmaf(nb < C1 ? x1[(long)b * C1 + nb] : x2[(long)b * C2 + (nb - C1)], g, sx);
  }
  dpos[i] = s;
  part[i] = sx;
  if (t == 0) dcls[d] = s;
}

// thread d: dw[d] and db[d], the sums over the band rows t = 1 .. T - 1 in order
__global__ void sf_embed_bwd_finish(int T, int D, const float* __restrict__ dpos, const float* __restrict__ part,
                                    float* __restrict__ dw, float* __restrict__ db) {
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= D) return;
  float sw = 0.f, sb = 0.f;
  for (int t = 1; t < T; ++t) {
    sw += part[t * D + d];
    sb += dpos[t * D + d];
  }
  dw[d] = sw;
  db[d] = sb;
}

}  // namespace

static bool fc_mode_ok(int mode) { return mode == VC_FC_PLAIN || mode == VC_FC_BN_RELU || mode == VC_FC_SIGMOID; }

VC_API int vc_fc_fused_fwd(int mode, int train, int B, int K, int N, const float* x, long ldx, const float* W,
                           const float* bias, const float* gamma, const float* beta, float* run_mean, float* run_var,
                           float eps, float momentum, float* y, long ldy, float* xhat, float* save_mean,
                           float* save_rstd, hipStream_t stream) {
  VC_REQUIRE(fc_mode_ok(mode) && (train == 0 || train == 1));
  VC_REQUIRE(B > 0 && K > 0 && K <= FC_KMAX && N > 0 && ldx >= K && ldy >= N);
  const bool bn = mode == VC_FC_BN_RELU, bnt = bn && train;
  if (bnt) VC_REQUIRE(B >= 2 && B <= FC_BMAX);   // one workgroup holds every row of its columns
  VC_REQUIRE_I32((long)B * std::max(ldx, ldy));
  VC_REQUIRE_I32((long)B * N);
  VC_REQUIRE(x && W && bias && y);
  if (bn) VC_REQUIRE(gamma && beta && run_mean && run_var && eps > 0.f && (save_mean != nullptr) == (save_rstd != nullptr));
  if (bnt) VC_REQUIRE(xhat && save_mean && momentum >= 0.f && momentum <= 1.f);
  const int RT = bnt ? B : FC_RT;
  hipLaunchKernelGGL(fc_fused_fwd, dim3(vc_cdiv(N, FC_NC), bnt ? 1 : vc_cdiv(B, FC_RT)), dim3(256), 0, stream, mode,
                     train, B, K, N, RT, x, ldx, W, bias, gamma, beta, run_mean, run_var, eps, momentum, y, ldy, xhat,
                     save_mean, save_rstd);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

VC_API int vc_fc_fused_bwd(int mode, int train, int B, int K, int N, const float* dy, long lddy, const float* y,
                           long ldy, const float* xhat, const float* x, long ldx, const float* gamma,
                           const float* rstd, float* dz, long lddz, float* dW, float* db, float* dgamma, float* dbeta,
                           hipStream_t stream) {
  VC_REQUIRE(fc_mode_ok(mode) && (train == 0 || train == 1));
  VC_REQUIRE(B > 0 && B <= FC_BMAX && K > 0 && K <= FC_KMAX && N > 0 && ldx >= K && lddy >= N);
  VC_REQUIRE(mode == VC_FC_PLAIN || ldy >= N);
  VC_REQUIRE(dz == nullptr || lddz >= N);
  VC_REQUIRE_I32((long)B * std::max(std::max(ldx, ldy), std::max(lddy, lddz)));
  VC_REQUIRE(dy && x && dW && db && (mode == VC_FC_PLAIN || y));
  if (mode == VC_FC_BN_RELU) VC_REQUIRE(xhat && gamma && rstd && dgamma && dbeta);
  hipLaunchKernelGGL(fc_fused_bwd, dim3(vc_cdiv(N, FC_NC)), dim3(256), 0, stream, mode, train, B, K, N, dy, lddy, y, ldy,
                     xhat, x, ldx, gamma, rstd, dz, lddz, dW, db, dgamma, dbeta);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

VC_API int vc_endnet_loss_fwd_bwd(int B, int ncls, int C1, int C2, const float* out, const long long* target,
                                  const float* weight, const float* de1, const float* x1, const float* de2,
                                  const float* x2, float* loss, float* dout, float* dde1, float* dde2,
                                  hipStream_t stream) {
  VC_REQUIRE(B > 0 && ncls > 0 && C1 > 0 && C2 > 0);
  VC_REQUIRE_I32((long)B * std::max(ncls, std::max(C1, C2)));
  VC_REQUIRE(out && target && de1 && x1 && de2 && x2 && loss && dout && dde1 && dde2);
  hipLaunchKernelGGL(endnet_loss, dim3(1), dim3(ELT), 0, stream, B, ncls, C1, C2, out, target, weight, de1, x1, de2, x2,
                     loss, dout, dde1, dde2);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

static int sf_embed_fwd_launch(int B, int C1, int C2, int D, const float* x1, const float* x2, const float* w,
                               const float* bias, const float* cls, const float* pos, float p, unsigned long long seed,
                               const unsigned long long* seed_dev, float* X, unsigned char* mask, hipStream_t stream) {
  VC_REQUIRE(B > 0 && C1 > 0 && C2 >= 0 && D > 0 && p >= 0.f && p < 1.f);
  const long total = (long)B * (C1 + C2 + 1) * D;
  VC_REQUIRE_I32(total);
  VC_REQUIRE(x1 && (x2 || C2 == 0) && w && bias && cls && pos && X && (p == 0.f || mask));
  hipLaunchKernelGGL(sf_embed_fwd, dim3(vc_cdiv(total, 256)), dim3(256), 0, stream, (int)total, make_fastdiv(D),
                     make_fastdiv(C1 + C2 + 1), C1, C2, x1, x2, w, bias, cls, pos, p, 1.0f / (1.0f - p), seed, seed_dev,
                     X, mask);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

VC_API int vc_sf_embed_fwd(int B, int C1, int C2, int D, const float* x1, const float* x2, const float* w,
                           const float* bias, const float* cls, const float* pos, float p, unsigned long long seed,
                           float* X, unsigned char* mask, hipStream_t stream) {
  return sf_embed_fwd_launch(B, C1, C2, D, x1, x2, w, bias, cls, pos, p, seed, nullptr, X, mask, stream);
}

VC_API int vc_sf_embed_fwd_ds(int B, int C1, int C2, int D, const float* x1, const float* x2, const float* w,
                              const float* bias, const float* cls, const float* pos, float p,
                              const unsigned long long* seed_dev, unsigned long long site_offset, float* X,
                              unsigned char* mask, hipStream_t stream) {
  VC_REQUIRE(seed_dev);
  return sf_embed_fwd_launch(B, C1, C2, D, x1, x2, w, bias, cls, pos, p, site_offset, seed_dev, X, mask, stream);
}

VC_API int vc_sf_embed_bwd(int B, int C1, int C2, int D, const float* x1, const float* x2, const float* dX,
                           const unsigned char* mask, float p, float* dw, float* db, float* dpos, float* dcls, float* ws,
                           long ws_floats, hipStream_t stream) {
  VC_REQUIRE(B > 0 && C1 > 0 && C2 >= 0 && D > 0 && p >= 0.f && p < 1.f);
  const int T = C1 + C2 + 1;
  const long TD = (long)T * D;
  VC_REQUIRE_I32((long)B * TD);
  VC_REQUIRE(x1 && (x2 || C2 == 0) && dX && dw && db && dpos && dcls && ws && ws_floats >= TD && (p == 0.f || mask));
  hipLaunchKernelGGL(sf_embed_bwd_cols, dim3(vc_cdiv(TD, 256)), dim3(256), 0, stream, (int)TD, D, B, C1, C2, x1, x2, dX,
                     p > 0.f ? mask : nullptr, 1.0f / (1.0f - p), dpos, dcls, ws);
  VC_CHECK_LAUNCH();
  hipLaunchKernelGGL(sf_embed_bwd_finish, dim3(vc_cdiv(D, 64)), dim3(64), 0, stream, T, D, dpos, ws, dw, db);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

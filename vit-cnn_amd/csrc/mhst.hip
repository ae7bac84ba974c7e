// MHST (model/compare_method/MHST/): the kernels behind vitcnn_amd/mhst.py.  Formulas: include/vitcnn.h.
// The 3x3x3 convolution is an implicit GEMM on the fp32 MFMA, and the head-select chain gate -> head mask -> pooling ->
// attention -> head mask is one fused kernel per direction (a block per (sample, head), its rows and probabilities in
// LDS).  The other kernels are direct fp32 forms with one owner per output: a grouped 3-D convolution family that also
// serves the pyramidal 2-D convolutions, the fusion / token embedding, the dual-softmax tail, and the chain's single
// steps (gate, head masks, pooling, attention), which the MLP's mask and the per-step tests use.  All sums run in a
// fixed order.
#include "common.h"

namespace {

constexpr int T = 65;     // tokens: cls + the 8 x 8 grid
constexpr int DM = 64;    // model width
constexpr int NH = 16;    // heads
constexpr int HD = 4;     // head width

__device__ __forceinline__ uint32_t mix32(uint64_t seed, uint32_t i) {   // vc_dropout_fwd's hash (s2eft.hip)
  uint64_t z = seed ^ ((uint64_t)i * 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (uint32_t)((z ^ (z >> 31)) >> 32);
}

struct ConvShape {
  int B, D, H, W, C, O, G, KD, KS, sd, pd, Dout;
};

// ------------------------------------------------------------------ grouped 3-D convolution
// one thread per output element (row, o), o fastest: a wave's lanes share x (broadcast) and walk 16+ weights
__global__ __launch_bounds__(256) void conv_fwd(ConvShape s, long total, const float* __restrict__ x, long ldx,
                                                const float* __restrict__ w, const float* __restrict__ bias,
                                                float* __restrict__ y, long ldy) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int o = (int)(idx % s.O);
  long row = idx / s.O;
  const int ww = (int)(row % s.W);
  long r = row / s.W;
  const int hh = (int)(r % s.H);
  r /= s.H;
  const int e = (int)(r % s.Dout);
  const int b = (int)(r / s.Dout);
  const int cg = s.C / s.G, og = s.O / s.G, g = o / og, ps = s.KS / 2, KK = s.KS * s.KS;
  const long wstride = (long)s.KD * KK;
  float acc = bias ? bias[o] : 0.f;
  for (int kd = 0; kd < s.KD; ++kd) {
    const int d = e * s.sd - s.pd + kd;
    if (d < 0 || d >= s.D) continue;
    for (int kh = 0; kh < s.KS; ++kh) {
      const int h = hh - ps + kh;
      if (h < 0 || h >= s.H) continue;
      for (int kw = 0; kw < s.KS; ++kw) {
        const int v = ww - ps + kw;
        if (v < 0 || v >= s.W) continue;
        const float* xp = x + ((((long)b * s.D + d) * s.H + h) * s.W + v) * ldx + g * cg;
        const float* wp = w + ((long)o * cg * s.KD + kd) * KK + kh * s.KS + kw;
        for (int c = 0; c < cg; ++c) acc += xp[c] * wp[c * wstride];
      }
    }
  }
  y[row * ldy + o] = acc;
}

// one thread per input element (row, c)
__global__ __launch_bounds__(256) void conv_dgrad(ConvShape s, long total, const float* __restrict__ dy, long lddy,
                                                  const float* __restrict__ w, float* __restrict__ dx, long lddx,
                                                  float beta) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c = (int)(idx % s.C);
  long row = idx / s.C;
  const int ww = (int)(row % s.W);
  long r = row / s.W;
  const int hh = (int)(r % s.H);
  r /= s.H;
  const int d = (int)(r % s.D);
  const int b = (int)(r / s.D);
  const int cg = s.C / s.G, og = s.O / s.G, g = c / cg, cl = c - g * cg, ps = s.KS / 2, KK = s.KS * s.KS;
  const long ostride = (long)cg * s.KD * KK;
  float acc = 0.f;
  for (int kd = 0; kd < s.KD; ++kd) {
    const int t = d + s.pd - kd;
    if (t < 0 || t % s.sd) continue;
    const int e = t / s.sd;
    if (e >= s.Dout) continue;
    for (int kh = 0; kh < s.KS; ++kh) {
      const int h = hh + ps - kh;
      if (h < 0 || h >= s.H) continue;
      for (int kw = 0; kw < s.KS; ++kw) {
        const int v = ww + ps - kw;
        if (v < 0 || v >= s.W) continue;
        const float* dp = dy + ((((long)b * s.Dout + e) * s.H + h) * s.W + v) * lddy + g * og;
        const float* wp = w + (((long)g * og * cg + cl) * s.KD + kd) * KK + kh * s.KS + kw;
        for (int oo = 0; oo < og; ++oo) acc += dp[oo] * wp[oo * ostride];
      }
    }
  }
  float* out = dx + row * lddx + c;
  *out = (beta != 0.f ? beta * *out : 0.f) + acc;
}

// One block of 8 waves per (group, input channel of the group, tap), then one per bias element.  A lane owns one of the
// H W <= 64 spatial positions (its shifted input position is loop-invariant), the block's waves split the (sample, depth)
// pairs, and every x value read serves the group's O / G <= 16 outputs, whose dy values are one contiguous run per lane.
// Per output: the wave's xor tree, then the 8 waves summed in wave order.
constexpr int WG_WAVES = 8;
constexpr int WG_OG = 16;

__global__ __launch_bounds__(64 * WG_WAVES) void conv_wgrad(ConvShape s, long nItems, const float* __restrict__ x,
                                                            long ldx, const float* __restrict__ dy, long lddy,
                                                            float* __restrict__ dw, float* __restrict__ db) {
  __shared__ float part[WG_WAVES][WG_OG];
  const long item = blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int HW = s.H * s.W;
  const long pairs = (long)s.B * s.Dout;
  if (item >= nItems) {   // bias: the column sum of dy
    const int o = (int)(item - nItems);
    const long rows = pairs * HW;
    float acc = 0.f;
    for (long r = threadIdx.x; r < rows; r += 64 * WG_WAVES) acc += dy[r * lddy + o];
    acc = wave_sum(acc);
    if (lane == 0) part[wave][0] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
      float t = 0.f;
      for (int w = 0; w < WG_WAVES; ++w) t += part[w][0];
      db[o] = t;
    }
    return;
  }
  const int cg = s.C / s.G, og = s.O / s.G, ps = s.KS / 2;
  long q = item;
  const int kw = (int)(q % s.KS);
  q /= s.KS;
  const int kh = (int)(q % s.KS);
  q /= s.KS;
  const int kd = (int)(q % s.KD);
  q /= s.KD;
  const int cl = (int)(q % cg);
  const int g = (int)(q / cg);
  const int c = g * cg + cl;
  const int hh = lane / s.W, ww = lane - hh * s.W;
  const int h = hh - ps + kh, v = ww - ps + kw;
  const bool valid = lane < HW && h >= 0 && h < s.H && v >= 0 && v < s.W;
  float acc[WG_OG];
#pragma unroll
  for (int oo = 0; oo < WG_OG; ++oo) acc[oo] = 0.f;
  if (valid) {
    const long xoff = (long)(h * s.W + v) * ldx + c;
    for (long n = wave; n < pairs; n += WG_WAVES) {
      const long b = n / s.Dout;
      const int d = (int)(n - b * s.Dout) * s.sd - s.pd + kd;
      if (d < 0 || d >= s.D) continue;
      const float xv = x[(b * s.D + d) * HW * ldx + xoff];
      const float* dp = dy + (n * HW + lane) * lddy + g * og;
#pragma unroll
      for (int oo = 0; oo < WG_OG; ++oo)
        if (oo < og) acc[oo] += xv * dp[oo];
    }
  }
#pragma unroll
  for (int oo = 0; oo < WG_OG; ++oo) {
    const float t = wave_sum(acc[oo]);
    if (lane == 0) part[wave][oo] = t;
  }
  __syncthreads();
  if (threadIdx.x < og) {
    const int oo = threadIdx.x;
    float t = 0.f;
    for (int w = 0; w < WG_WAVES; ++w) t += part[w][oo];
    dw[((((long)(g * og + oo) * cg + cl) * s.KD + kd) * s.KS + kh) * s.KS + kw] = t;
  }
}

// ------------------------------------------------------------------ the 3x3x3 conv 16 -> 16 on the MFMA
// Implicit GEMM on v_mfma_f32_16x16x4_f32 (A: row = lane & 15, k = lane >> 4; B: col = lane & 15, k = lane >> 4;
// D: col = lane & 15, row = (lane >> 4) * 4 + r), K = 27 taps x 16 channels walked tap-major, N = 16.
// Forward and data gradient are one kernel: a block owns one (sample, depth) plane of 64 positions, a wave 16 of them;
// the weight sits in LDS as [tap][k][n] (forward: k = c, n = o; data gradient: k = o, n = c, the tap offset mirrored).
// A lane reads the 4 channels 4 kq .. 4 kq + 3 of its position's neighbour as one float4 and feeds them to 4 MFMAs
// whose k index kq stands for channel 4 kq + j on both operands.
constexpr int C3 = 16, C3_TAPS = 27, C3_W = C3 * C3 * C3_TAPS;

template <int MODE>
__global__ __launch_bounds__(256) void conv3_mfma(int D, const float* __restrict__ in, long ldi,
                                                  const float* __restrict__ w, const float* __restrict__ bias,
                                                  float* __restrict__ out, long ldo, float beta) {
  __shared__ float wl[C3_TAPS * C3 * C3];
  for (int i = threadIdx.x; i < C3_W; i += 256) {   // w is [o][c][tap]
    const int o = i / (C3 * C3_TAPS), c = (i / C3_TAPS) % C3, t = i % C3_TAPS;
    const int k = MODE == 0 ? c : o, n = MODE == 0 ? o : c;
    wl[(t * C3 + k) * C3 + n] = w[i];
  }
  __syncthreads();
  const int plane = blockIdx.x, b = plane / D, d = plane - b * D;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, m = lane & 15, kq = lane >> 4;
  const int pos = wave * 16 + m, h = pos >> 3, v = pos & 7;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kd = 0; kd < 3; ++kd) {
    const int dd = MODE == 0 ? d + kd - 1 : d + 1 - kd;
    if (dd < 0 || dd >= D) continue;   // uniform over the block
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      const int hh = MODE == 0 ? h + kh - 1 : h + 1 - kh;
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int vv = MODE == 0 ? v + kw - 1 : v + 1 - kw;
        const int t = kd * 9 + kh * 3 + kw;
        f32x4 a = {0.f, 0.f, 0.f, 0.f};
        if (hh >= 0 && hh < 8 && vv >= 0 && vv < 8)
          a = *reinterpret_cast<const f32x4*>(in + (((long)b * D + dd) * 64 + hh * 8 + vv) * ldi + 4 * kq);
        const float* wt = wl + (t * C3 + 4 * kq) * C3 + m;
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], wt[j * C3], acc, 0, 0, 0);
      }
    }
  }
  const float bv = bias ? bias[m] : 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float* o = out + ((long)plane * 64 + wave * 16 + kq * 4 + r) * ldo + m;
    *o = (beta != 0.f ? beta * *o : 0.f) + acc[r] + bv;
  }
}

// Weight gradient: D[o][c] of tap t += dy[row][o] x[neighbour(row, t)][c] with the rows as k, 4 per MFMA.  One wave
// per block walks the planes blockIdx.x, + gridDim.x, ... in order with 27 accumulators and leaves its partial
// [o][c][tap] in ws; the partials are then summed in block order (sum_rows_kernel): a fixed order.
__global__ __launch_bounds__(64) void conv3_wgrad_mfma(int planes, int D, const float* __restrict__ x, long ldx,
                                                       const float* __restrict__ dy, long lddy,
                                                       float* __restrict__ part) {
  const int lane = threadIdx.x, n = lane & 15, kq = lane >> 4;
  f32x4 acc[C3_TAPS];
#pragma unroll
  for (int t = 0; t < C3_TAPS; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int plane = blockIdx.x; plane < planes; plane += gridDim.x) {
    const int b = plane / D, d = plane - b * D;
    for (int step = 0; step < 16; ++step) {
      const int pos = step * 4 + kq, h = pos >> 3, v = pos & 7;
      const float a = dy[((long)plane * 64 + pos) * lddy + n];
#pragma unroll
      for (int kd = 0; kd < 3; ++kd) {
        const int dd = d + kd - 1;
        const bool dok = dd >= 0 && dd < D;
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
          const int hh = h + kh - 1;
#pragma unroll
          for (int kw = 0; kw < 3; ++kw) {
            const int vv = v + kw - 1;
            float bv = 0.f;
            if (dok && hh >= 0 && hh < 8 && vv >= 0 && vv < 8) bv = x[(((long)b * D + dd) * 64 + hh * 8 + vv) * ldx + n];
            acc[kd * 9 + kh * 3 + kw] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv, acc[kd * 9 + kh * 3 + kw], 0, 0, 0);
          }
        }
      }
    }
  }
  float* pr = part + (long)blockIdx.x * C3_W;
#pragma unroll
  for (int t = 0; t < C3_TAPS; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) pr[((kq * 4 + r) * C3 + n) * C3_TAPS + t] = acc[t][r];
}

// ------------------------------------------------------------------ fusion + token embedding
__global__ __launch_bounds__(256) void embed_fwd(const float* __restrict__ ph, const float* __restrict__ pl,
                                                 const float* __restrict__ wh, const float* __restrict__ wl,
                                                 const float* __restrict__ W, const float* __restrict__ bias,
                                                 const float* __restrict__ pos, const float* __restrict__ cls,
                                                 float* __restrict__ xcnn, float* __restrict__ X0) {
  __shared__ float f[16][DM];
  const int b = blockIdx.x;
  const float a = *wh, c2 = *wl;
  for (int i = threadIdx.x; i < 16 * DM; i += 256)
    f[i / DM][i % DM] = a * ph[(long)b * 16 * DM + i] + c2 * pl[(long)b * 16 * DM + i];
  __syncthreads();
  for (int i = threadIdx.x; i < DM * DM; i += 256) {
    const int j = i / DM, c = i % DM;
    float acc = 0.f;
#pragma unroll
    for (int p = 0; p < 16; ++p) acc += W[j * 16 + p] * f[p][c];
    acc += bias[j];
    xcnn[(long)b * DM * DM + i] = acc;
    X0[((long)b * T + 1 + j) * DM + c] = acc + pos[(1 + j) * DM + c] + pos[c];
  }
  if (threadIdx.x < DM) X0[(long)b * T * DM + threadIdx.x] = cls[threadIdx.x] + pos[threadIdx.x];
}

__global__ __launch_bounds__(256) void embed_bwd(const float* __restrict__ ph, const float* __restrict__ pl,
                                                 const float* __restrict__ wh, const float* __restrict__ wl,
                                                 const float* __restrict__ W, const float* __restrict__ dX0,
                                                 const float* __restrict__ dxcnn, float* __restrict__ dph,
                                                 float* __restrict__ dpl, float* __restrict__ part) {
  __shared__ float f[16][DM];
  __shared__ float g[DM][DM + 1];
  __shared__ float df[16][DM];
  __shared__ float ch[2][DM];
  const int b = blockIdx.x;
  const float a = *wh, c2 = *wl;
  float* pr = part + (long)b * VC_MHST_EMBED_PART;
  for (int i = threadIdx.x; i < 16 * DM; i += 256)
    f[i / DM][i % DM] = a * ph[(long)b * 16 * DM + i] + c2 * pl[(long)b * 16 * DM + i];
  for (int i = threadIdx.x; i < DM * DM; i += 256) {
    const int j = i / DM, c = i % DM;
    g[j][c] = dxcnn[(long)b * DM * DM + i] + dX0[((long)b * T + 1 + j) * DM + c];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < DM * 16; i += 256) {   // dW[j][p]
    const int j = i / 16, p = i % 16;
    float acc = 0.f;
    for (int c = 0; c < DM; ++c) acc += g[j][c] * f[p][c];
    pr[i] = acc;
  }
  if (threadIdx.x < DM) {   // dbias[j]; dpos0[c] = every row of dX0
    const int j = threadIdx.x;
    float acc = 0.f;
    for (int c = 0; c < DM; ++c) acc += g[j][c];
    pr[1024 + j] = acc;
    float ap = 0.f;
    for (int t = 0; t < T; ++t) ap += dX0[((long)b * T + t) * DM + j];
    pr[1088 + j] = ap;
  }
  for (int i = threadIdx.x; i < 16 * DM; i += 256) {   // df[p][c]
    const int p = i / DM, c = i % DM;
    float acc = 0.f;
    for (int j = 0; j < DM; ++j) acc += W[j * 16 + p] * g[j][c];
    df[p][c] = acc;
    dph[(long)b * 16 * DM + i] = a * acc;
    dpl[(long)b * 16 * DM + i] = c2 * acc;
  }
  __syncthreads();
  if (threadIdx.x < DM) {
    const int c = threadIdx.x;
    float sh = 0.f, sl = 0.f;
    for (int p = 0; p < 16; ++p) {
      sh += df[p][c] * ph[(long)b * 16 * DM + p * DM + c];
      sl += df[p][c] * pl[(long)b * 16 * DM + p * DM + c];
    }
    ch[0][c] = sh;
    ch[1][c] = sl;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    float acc = 0.f;
    for (int c = 0; c < DM; ++c) acc += ch[threadIdx.x][c];
    pr[1152 + threadIdx.x] = acc;
    pr[1154 + threadIdx.x] = 0.f;
  }
}

// ------------------------------------------------------------------ head gate
__global__ __launch_bounds__(256) void gate_fwd(int n, const float* __restrict__ X, long ldx, const float* __restrict__ Wg,
                                                const float* __restrict__ bg, const float* __restrict__ noise_in,
                                                int train, float inv_tau, unsigned long long seed,
                                                const unsigned long long* __restrict__ seed_dev,
                                                float* __restrict__ logits, float* __restrict__ noise_out,
                                                float* __restrict__ y, float* __restrict__ sel) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int b = i / NH, h = i % NH;
  const float* xr = X + (long)b * ldx;
  float acc = 0.f;
  for (int c = 0; c < DM; ++c) acc += Wg[h * DM + c] * xr[c];
  acc += bg[h];
  logits[i] = acc;
  float v = acc, nz = 0.f;
  if (train) {
    if (noise_in) {
      nz = noise_in[i];
    } else {
      // 23 bits + 0.5 is exact in fp32, so 0 < u < 1 strictly
      const float u = ((float)(mix32(vc_site_seed(seed, seed_dev), (uint32_t)i) >> 9) + 0.5f) * (1.0f / 8388608.0f);
      nz = logf(u) - log1pf(-u);
    }
    v = (acc + nz) * inv_tau;
  }
  if (noise_out) noise_out[i] = nz;
  y[i] = 1.0f / (1.0f + expf(-v));
  sel[i] = v > 0.f ? 1.f : 0.f;
}

__global__ __launch_bounds__(256) void gate_bwd(int n, const float* __restrict__ dsel, const float* __restrict__ y,
                                                float scale, float* __restrict__ dlogits) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float v = y[i];
  dlogits[i] = dsel[i] * v * (1.f - v) * scale;
}

// ------------------------------------------------------------------ head masks
__global__ __launch_bounds__(256) void headmask_fwd(long total, int Wd, const float* __restrict__ X,
                                                    const float* __restrict__ sel, float* __restrict__ Y) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % Wd);
  const long b = i / ((long)Wd * T);
  Y[i] = X[i] * sel[b * NH + (c % DM) / HD];
}

// one block per sample; thread c owns column c (Wd <= 192 < 256)
__global__ __launch_bounds__(256) void headmask_bwd(int Wd, const float* __restrict__ dY, const float* __restrict__ X,
                                                    const float* __restrict__ sel, float* __restrict__ dX,
                                                    float* __restrict__ dsel, float beta) {
  __shared__ float col[192];
  const int b = blockIdx.x, c = threadIdx.x;
  if (c < Wd) {
    const float sv = sel[b * NH + (c % DM) / HD];
    float acc = 0.f;
    for (int t = 0; t < T; ++t) {
      const long i = ((long)b * T + t) * Wd + c;
      const float d = dY[i];
      acc += d * X[i];
      dX[i] = d * sv;
    }
    col[c] = acc;
  }
  __syncthreads();
  if (c < NH) {
    float acc = 0.f;
    for (int s = 0; s < Wd / DM; ++s)
      for (int k = 0; k < HD; ++k) acc += col[s * DM + c * HD + k];
    float* out = dsel + b * NH + c;
    *out = (beta != 0.f ? beta * *out : 0.f) + acc;
  }
}

// ------------------------------------------------------------------ pooling of q | k | v
// the conv output of (token t, column col) of one tensor whose 65 x 64 block starts at x (row stride ld)
__device__ __forceinline__ float pool_conv(const float* x, long ld, int t, int col, const float* cw) {
  if (t == 0) return x[col];
  const int py = (t - 1) >> 3, px = (t - 1) & 7;
  const float* w = cw + (col & 3) * 9;
  float acc = 0.f;
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int yy = py + ky - 1;
    if (yy < 0 || yy > 7) continue;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int xx = px + kx - 1;
      if (xx < 0 || xx > 7) continue;
      acc += w[ky * 3 + kx] * x[(long)(1 + yy * 8 + xx) * ld + col];
    }
  }
  return acc;
}

__global__ __launch_bounds__(256) void pool_fwd(long total, const float* __restrict__ X, const float* __restrict__ pw,
                                                float eps, float* __restrict__ Y) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;   // (b, t, s, h)
  if (i >= total) return;
  const int h = (int)(i % NH);
  const int s = (int)((i / NH) % 3);
  const int t = (int)((i / (NH * 3)) % T);
  const long b = i / (NH * 3 * T);
  const float* p = pw + s * 44;
  const float* xb = X + b * T * 192 + s * DM;
  float c[HD];
  float mean = 0.f;
#pragma unroll
  for (int k = 0; k < HD; ++k) {
    c[k] = pool_conv(xb, 192, t, h * HD + k, p);
    mean += c[k];
  }
  mean *= 0.25f;
  float var = 0.f;
#pragma unroll
  for (int k = 0; k < HD; ++k) var += (c[k] - mean) * (c[k] - mean);
  const float rstd = rsqrtf(var * 0.25f + eps);
  float* yo = Y + (b * T + t) * 192 + s * DM + h * HD;
#pragma unroll
  for (int k = 0; k < HD; ++k) yo[k] = (c[k] - mean) * rstd * p[36 + k] + p[40 + k];
}

// one block per (sample, tensor)
__global__ __launch_bounds__(256) void pool_bwd(const float* __restrict__ X, const float* __restrict__ pw, float eps,
                                                const float* __restrict__ dY, float* __restrict__ dX,
                                                float* __restrict__ part) {
  __shared__ float xs[T][DM];
  __shared__ float dc[T][DM];
  __shared__ float pg[T][DM];
  __shared__ float hw[NH][36];
  __shared__ float colA[DM], colB[DM];
  const int b = blockIdx.x, s = blockIdx.y;
  const float* p = pw + s * 44;
  const float* xb = X + (long)b * T * 192 + s * DM;
  const float* dyb = dY + (long)b * T * 192 + s * DM;
  float* pr = part + (long)b * VC_MHST_POOL_FLOATS + s * 44;
  for (int i = threadIdx.x; i < T * DM; i += 256) xs[i / DM][i % DM] = xb[(long)(i / DM) * 192 + i % DM];
  __syncthreads();
  for (int i = threadIdx.x; i < T * NH; i += 256) {
    const int t = i / NH, h = i % NH;
    float c[HD], xh[HD], dxh[HD];
    float mean = 0.f;
#pragma unroll
    for (int k = 0; k < HD; ++k) {
      c[k] = pool_conv(&xs[0][0], DM, t, h * HD + k, p);
      mean += c[k];
    }
    mean *= 0.25f;
    float var = 0.f;
#pragma unroll
    for (int k = 0; k < HD; ++k) var += (c[k] - mean) * (c[k] - mean);
    const float rstd = rsqrtf(var * 0.25f + eps);
    float m1 = 0.f, m2 = 0.f;
#pragma unroll
    for (int k = 0; k < HD; ++k) {
      const float d = dyb[(long)t * 192 + h * HD + k];
      xh[k] = (c[k] - mean) * rstd;
      dxh[k] = d * p[36 + k];
      pg[t][h * HD + k] = d * xh[k];
      m1 += dxh[k];
      m2 += dxh[k] * xh[k];
    }
    m1 *= 0.25f;
    m2 *= 0.25f;
#pragma unroll
    for (int k = 0; k < HD; ++k) dc[t][h * HD + k] = rstd * (dxh[k] - m1 - xh[k] * m2);
  }
  __syncthreads();
  if (threadIdx.x < DM) {   // LayerNorm(4) parameter gradients: per column over t, then over the heads
    const int c = threadIdx.x;
    float a = 0.f, bb = 0.f;
    for (int t = 0; t < T; ++t) {
      a += pg[t][c];
      bb += dyb[(long)t * 192 + c];
    }
    colA[c] = a;
    colB[c] = bb;
  }
  for (int i = threadIdx.x; i < NH * 36; i += 256) {   // conv weight gradient per head
    const int h = i / 36, k = (i % 36) / 9, tap = i % 9, ky = tap / 3, kx = tap % 3;
    const int col = h * HD + k;
    float acc = 0.f;
    for (int pos = 0; pos < 64; ++pos) {
      const int yy = (pos >> 3) + ky - 1, xx = (pos & 7) + kx - 1;
      if (yy < 0 || yy > 7 || xx < 0 || xx > 7) continue;
      acc += dc[1 + pos][col] * xs[1 + yy * 8 + xx][col];
    }
    hw[h][i % 36] = acc;
  }
  __syncthreads();
  if (threadIdx.x < 36) {
    float acc = 0.f;
    for (int h = 0; h < NH; ++h) acc += hw[h][threadIdx.x];
    pr[threadIdx.x] = acc;
  } else if (threadIdx.x >= 64 && threadIdx.x < 72) {
    const int k = threadIdx.x & 3;
    const float* src = threadIdx.x < 68 ? colA : colB;
    float acc = 0.f;
    for (int h = 0; h < NH; ++h) acc += src[h * HD + k];
    pr[(threadIdx.x < 68 ? 36 : 40) + k] = acc;
  }
  for (int i = threadIdx.x; i < T * DM; i += 256) {   // dX: the transposed depthwise conv
    const int t = i / DM, col = i % DM;
    float acc;
    if (t == 0) {
      acc = dc[0][col];
    } else {
      const int py = (t - 1) >> 3, px = (t - 1) & 7;
      const float* w = p + (col & 3) * 9;
      acc = 0.f;
      for (int ky = 0; ky < 3; ++ky) {
        const int yy = py - ky + 1;
        if (yy < 0 || yy > 7) continue;
        for (int kx = 0; kx < 3; ++kx) {
          const int xx = px - kx + 1;
          if (xx < 0 || xx > 7) continue;
          acc += dc[1 + yy * 8 + xx][col] * w[ky * 3 + kx];
        }
      }
    }
    dX[((long)b * T + t) * 192 + s * DM + col] = acc;
  }
}

// ------------------------------------------------------------------ attention, 16 heads of width 4
__global__ __launch_bounds__(256) void attn_fwd(int total, const float* __restrict__ QKV, float scale, float p,
                                                unsigned long long seed, const unsigned long long* __restrict__ seed_dev,
                                                unsigned char* __restrict__ mask, float* __restrict__ O) {
  const int idx = blockIdx.x * 256 + threadIdx.x;   // (b, h, i)
  if (idx >= total) return;
  const int i = idx % T, h = (idx / T) % NH, b = idx / (T * NH);
  const float* base = QKV + (long)b * T * 192 + h * HD;
  const float* qp = base + (long)i * 192;
  const float q0 = qp[0], q1 = qp[1], q2 = qp[2], q3 = qp[3];
  float m = -INFINITY;
  for (int j = 0; j < T; ++j) {
    const float* k = base + (long)j * 192 + DM;
    m = fmaxf(m, scale * (q0 * k[0] + q1 * k[1] + q2 * k[2] + q3 * k[3]));
  }
  if (p > 0.f) seed = vc_site_seed(seed, seed_dev);
  float sum = 0.f, a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  for (int j = 0; j < T; ++j) {
    const float* k = base + (long)j * 192 + DM;
    const float* v = k + DM;
    const float e = expf(scale * (q0 * k[0] + q1 * k[1] + q2 * k[2] + q3 * k[3]) - m);
    sum += e;
    bool keep = true;
    if (p > 0.f) {
      const uint32_t mi = (uint32_t)idx * T + j;
      keep = (float)(mix32(seed, mi) >> 8) * (1.0f / 16777216.0f) >= p;
    }
    if (mask) mask[(long)idx * T + j] = keep ? 1 : 0;
    if (keep) {
      a0 += e * v[0];
      a1 += e * v[1];
      a2 += e * v[2];
      a3 += e * v[3];
    }
  }
  const float inv = 1.0f / (sum * (1.0f - p));
  const float r = i > 0 ? 1.f : 0.f;
  float* o = O + ((long)b * T + i) * DM + h * HD;
  o[0] = a0 * inv + r * q0;
  o[1] = a1 * inv + r * q1;
  o[2] = a2 * inv + r * q2;
  o[3] = a3 * inv + r * q3;
}

// one block per (sample, head): dS and the dropped probabilities of the head's 65 x 65 in LDS
__global__ __launch_bounds__(128) void attn_bwd(const float* __restrict__ QKV, float scale, float p,
                                                const unsigned char* __restrict__ mask, const float* __restrict__ dO,
                                                float* __restrict__ dQKV) {
  __shared__ float dS[T][T];
  __shared__ float Pd[T][T];
  __shared__ float q[T][HD], k[T][HD], v[T][HD], g[T][HD];
  const int b = blockIdx.x / NH, h = blockIdx.x % NH;
  const float* base = QKV + (long)b * T * 192 + h * HD;
  for (int i = threadIdx.x; i < T * HD; i += 128) {
    const int t = i / HD, c = i % HD;
    q[t][c] = base[(long)t * 192 + c];
    k[t][c] = base[(long)t * 192 + DM + c];
    v[t][c] = base[(long)t * 192 + 2 * DM + c];
    g[t][c] = dO[((long)b * T + t) * DM + h * HD + c];
  }
  __syncthreads();
  const float ks = 1.0f / (1.0f - p);
  const int i = threadIdx.x;
  if (i < T) {
    const unsigned char* mr = mask ? mask + ((long)blockIdx.x * T + i) * T : nullptr;
    float m = -INFINITY;
    for (int j = 0; j < T; ++j)
      m = fmaxf(m, scale * (q[i][0] * k[j][0] + q[i][1] * k[j][1] + q[i][2] * k[j][2] + q[i][3] * k[j][3]));
    float sum = 0.f;
    for (int j = 0; j < T; ++j) {
      const float e = expf(scale * (q[i][0] * k[j][0] + q[i][1] * k[j][1] + q[i][2] * k[j][2] + q[i][3] * k[j][3]) - m);
      Pd[i][j] = e;
      sum += e;
    }
    const float inv = 1.0f / sum;
    float rowdot = 0.f;
    for (int j = 0; j < T; ++j) {
      const float pr = Pd[i][j] * inv;
      const float kp = (mr ? (mr[j] ? ks : 0.f) : 1.f);
      const float dP = (g[i][0] * v[j][0] + g[i][1] * v[j][1] + g[i][2] * v[j][2] + g[i][3] * v[j][3]) * kp;
      Pd[i][j] = pr;
      dS[i][j] = dP;
      rowdot += pr * dP;
    }
    float d0 = 0.f, d1 = 0.f, d2 = 0.f, d3 = 0.f;
    for (int j = 0; j < T; ++j) {
      const float pr = Pd[i][j];
      const float ds = pr * (dS[i][j] - rowdot);
      dS[i][j] = ds;
      Pd[i][j] = pr * (mr ? (mr[j] ? ks : 0.f) : 1.f);
      d0 += ds * k[j][0];
      d1 += ds * k[j][1];
      d2 += ds * k[j][2];
      d3 += ds * k[j][3];
    }
    const float r = i > 0 ? 1.f : 0.f;
    float* o = dQKV + ((long)b * T + i) * 192 + h * HD;
    o[0] = scale * d0 + r * g[i][0];
    o[1] = scale * d1 + r * g[i][1];
    o[2] = scale * d2 + r * g[i][2];
    o[3] = scale * d3 + r * g[i][3];
  }
  __syncthreads();
  if (i < T) {   // thread j = i: dk_j, dv_j over the rows in ascending order
    const int j = i;
    float k0 = 0.f, k1 = 0.f, k2 = 0.f, k3 = 0.f, v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f;
    for (int r = 0; r < T; ++r) {
      const float ds = dS[r][j], pd = Pd[r][j];
      k0 += ds * q[r][0];
      k1 += ds * q[r][1];
      k2 += ds * q[r][2];
      k3 += ds * q[r][3];
      v0 += pd * g[r][0];
      v1 += pd * g[r][1];
      v2 += pd * g[r][2];
      v3 += pd * g[r][3];
    }
    float* o = dQKV + ((long)b * T + j) * 192 + h * HD;
    o[DM + 0] = scale * k0;
    o[DM + 1] = scale * k1;
    o[DM + 2] = scale * k2;
    o[DM + 3] = scale * k3;
    o[2 * DM + 0] = v0;
    o[2 * DM + 1] = v1;
    o[2 * DM + 2] = v2;
    o[2 * DM + 3] = v3;
  }
}

// ------------------------------------------------------------------ the fused head-select attention
// gate -> head mask -> pooling of q | k | v -> attention -> head mask on the output, one block per (sample, head): every
// step of that chain is independent per head (the pooling conv is depthwise, its LayerNorm per head row), so a block
// holds its head's masked q | k | v columns [3][65][4] and their pooled form in LDS and nothing of the chain but the
// masked attention output goes to HBM.  The backward recomputes the chain from the raw q | k | v, holds the head's 65 x 65
// dS and dropped probabilities in LDS (33.8 KB), and leaves the pooling parameters' gradients as one partial row per
// (sample, head), summed by the caller in a fixed order.
constexpr int HS_THREADS = 128;

struct HsGate {
  float v, y, sel, noise;
};

// one head's pooled rows from its masked rows xr [3][T][HD] -> pq [3][T][HD] (all threads; no barrier inside)
__device__ __forceinline__ void hs_pool(const float (*xr)[T][HD], float (*pq)[T][HD], const float* __restrict__ pw,
                                        float eps) {
  for (int i = threadIdx.x; i < 3 * T; i += HS_THREADS) {
    const int s = i / T, t = i - s * T;
    const float* p = pw + s * 44;
    float c[HD], mean = 0.f;
#pragma unroll
    for (int k = 0; k < HD; ++k) {
      c[k] = pool_conv(&xr[s][0][0], HD, t, k, p);
      mean += c[k];
    }
    mean *= 0.25f;
    float var = 0.f;
#pragma unroll
    for (int k = 0; k < HD; ++k) var += (c[k] - mean) * (c[k] - mean);
    const float rstd = rsqrtf(var * 0.25f + eps);
#pragma unroll
    for (int k = 0; k < HD; ++k) pq[s][t][k] = (c[k] - mean) * rstd * p[36 + k] + p[40 + k];
  }
}

__global__ __launch_bounds__(HS_THREADS) void hsattn_fwd(
    const float* __restrict__ X, long ldx, const float* __restrict__ Wg, const float* __restrict__ bg,
    const float* __restrict__ noise_in, int train, float inv_tau, unsigned long long seed_gate,
    unsigned long long seed_prob, const unsigned long long* __restrict__ seed_dev, const float* __restrict__ QKV,
    const float* __restrict__ pw, float eps, float scale, float p, unsigned char* __restrict__ mask,
    float* __restrict__ logits, float* __restrict__ noise_out, float* __restrict__ y, float* __restrict__ sel,
    float* __restrict__ AM) {
  __shared__ float xr[3][T][HD];
  __shared__ float pq[3][T][HD];
  __shared__ float s_sel;
  const int b = blockIdx.x / NH, h = blockIdx.x % NH, tid = threadIdx.x;
  if (tid < 64) {   // the gate of this head: Linear(64, 16) row h on the cls row, noise, threshold
    float t = wave_sum(Wg[h * DM + tid] * X[(long)b * ldx + tid]);
    if (tid == 0) {
      t += bg[h];
      float v = t, nz = 0.f;
      if (train) {
        if (noise_in) {
          nz = noise_in[blockIdx.x];
        } else {
          const float u = ((float)(mix32(vc_site_seed(seed_gate, seed_dev), (uint32_t)blockIdx.x) >> 9) + 0.5f) *
                          (1.0f / 8388608.0f);
          nz = logf(u) - log1pf(-u);
        }
        v = (t + nz) * inv_tau;
      }
      const float sv = v > 0.f ? 1.f : 0.f;
      logits[blockIdx.x] = t;
      if (noise_out) noise_out[blockIdx.x] = nz;
      y[blockIdx.x] = 1.0f / (1.0f + expf(-v));
      sel[blockIdx.x] = sv;
      s_sel = sv;
    }
  }
  __syncthreads();
  const float sv = s_sel;
  for (int i = tid; i < 3 * T * HD; i += HS_THREADS) {
    const int s = i / (T * HD), t = (i / HD) % T, c = i % HD;
    xr[s][t][c] = QKV[((long)b * T + t) * 192 + s * DM + h * HD + c] * sv;
  }
  __syncthreads();
  hs_pool(xr, pq, pw, eps);
  __syncthreads();
  const int i = tid;
  if (i < T) {
    const float q0 = pq[0][i][0], q1 = pq[0][i][1], q2 = pq[0][i][2], q3 = pq[0][i][3];
    float m = -INFINITY;
    for (int j = 0; j < T; ++j)
      m = fmaxf(m, scale * (q0 * pq[1][j][0] + q1 * pq[1][j][1] + q2 * pq[1][j][2] + q3 * pq[1][j][3]));
    unsigned long long sp = seed_prob;
    if (p > 0.f) sp = vc_site_seed(seed_prob, seed_dev);
    const long row = (long)blockIdx.x * T + i;
    float sum = 0.f, a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int j = 0; j < T; ++j) {
      const float e =
          expf(scale * (q0 * pq[1][j][0] + q1 * pq[1][j][1] + q2 * pq[1][j][2] + q3 * pq[1][j][3]) - m);
      sum += e;
      bool keep = true;
      if (p > 0.f) keep = (float)(mix32(sp, (uint32_t)(row * T + j)) >> 8) * (1.0f / 16777216.0f) >= p;
      if (mask) mask[row * T + j] = keep ? 1 : 0;
      if (keep) {
        a0 += e * pq[2][j][0];
        a1 += e * pq[2][j][1];
        a2 += e * pq[2][j][2];
        a3 += e * pq[2][j][3];
      }
    }
    const float inv = 1.0f / (sum * (1.0f - p));
    const float r = i > 0 ? 1.f : 0.f;
    float* o = AM + ((long)b * T + i) * DM + h * HD;
    o[0] = (a0 * inv + r * q0) * sv;
    o[1] = (a1 * inv + r * q1) * sv;
    o[2] = (a2 * inv + r * q2) * sv;
    o[3] = (a3 * inv + r * q3) * sv;
  }
}

__global__ __launch_bounds__(HS_THREADS) void hsattn_bwd(
    const float* __restrict__ QKV, const float* __restrict__ sel, const float* __restrict__ yg,
    const float* __restrict__ pw, float eps, float scale, float p, const unsigned char* __restrict__ mask,
    const float* __restrict__ dAM, const float* __restrict__ dsel_in, float gscale, float* __restrict__ dQKV,
    float* __restrict__ part, float* __restrict__ dlogits) {
  __shared__ float dS[T][T];
  __shared__ float Pd[T][T];
  __shared__ float xr[3][T][HD];    // masked q | k | v of the head
  __shared__ float pq[3][T][HD];    // pooled
  __shared__ float dqp[3][T][HD];   // gradient of the pooled rows
  __shared__ float dc[3][T][HD];    // gradient of the conv output
  __shared__ float pgx[3][T][HD];   // dy * xhat (LayerNorm weight gradient terms)
  __shared__ float g[T][HD];        // gradient of the unmasked attention output
  __shared__ float red[HS_THREADS + T];
  const int b = blockIdx.x / NH, h = blockIdx.x % NH, tid = threadIdx.x;
  const float sv = sel[blockIdx.x];
  for (int i = tid; i < 3 * T * HD; i += HS_THREADS) {
    const int s = i / (T * HD), t = (i / HD) % T, c = i % HD;
    xr[s][t][c] = QKV[((long)b * T + t) * 192 + s * DM + h * HD + c] * sv;
  }
  __syncthreads();
  hs_pool(xr, pq, pw, eps);
  __syncthreads();
  const float ks = 1.0f / (1.0f - p);
  const int i = tid;
  if (i < T) {   // row i: the probabilities again, the output again (the mask's gradient needs it), dS, dq
    const unsigned char* mr = mask ? mask + ((long)blockIdx.x * T + i) * T : nullptr;
    const float* dam = dAM + ((long)b * T + i) * DM + h * HD;
    const float d0 = dam[0], d1 = dam[1], d2 = dam[2], d3 = dam[3];
    const float g0 = d0 * sv, g1 = d1 * sv, g2 = d2 * sv, g3 = d3 * sv;
    g[i][0] = g0;
    g[i][1] = g1;
    g[i][2] = g2;
    g[i][3] = g3;
    const float q0 = pq[0][i][0], q1 = pq[0][i][1], q2 = pq[0][i][2], q3 = pq[0][i][3];
    float m = -INFINITY;
    for (int j = 0; j < T; ++j)
      m = fmaxf(m, scale * (q0 * pq[1][j][0] + q1 * pq[1][j][1] + q2 * pq[1][j][2] + q3 * pq[1][j][3]));
    float sum = 0.f;
    for (int j = 0; j < T; ++j) {
      const float e =
          expf(scale * (q0 * pq[1][j][0] + q1 * pq[1][j][1] + q2 * pq[1][j][2] + q3 * pq[1][j][3]) - m);
      Pd[i][j] = e;
      sum += e;
    }
    const float inv = 1.0f / sum;
    float rowdot = 0.f, o0 = 0.f, o1 = 0.f, o2 = 0.f, o3 = 0.f;
    for (int j = 0; j < T; ++j) {
      const float pr = Pd[i][j] * inv;
      const float kp = mr ? (mr[j] ? ks : 0.f) : 1.f;
      const float dP = (g0 * pq[2][j][0] + g1 * pq[2][j][1] + g2 * pq[2][j][2] + g3 * pq[2][j][3]) * kp;
      const float pd = pr * kp;
      o0 += pd * pq[2][j][0];
      o1 += pd * pq[2][j][1];
      o2 += pd * pq[2][j][2];
      o3 += pd * pq[2][j][3];
      Pd[i][j] = pr;
      dS[i][j] = dP;
      rowdot += pr * dP;
    }
    const float r = i > 0 ? 1.f : 0.f;
    // d sel through the output mask: dAM . (unmasked output)
    red[HS_THREADS + i] = d0 * (o0 + r * q0) + d1 * (o1 + r * q1) + d2 * (o2 + r * q2) + d3 * (o3 + r * q3);
    float e0 = 0.f, e1 = 0.f, e2 = 0.f, e3 = 0.f;
    for (int j = 0; j < T; ++j) {
      const float pr = Pd[i][j];
      const float ds = pr * (dS[i][j] - rowdot);
      dS[i][j] = ds;
      Pd[i][j] = pr * (mr ? (mr[j] ? ks : 0.f) : 1.f);
      e0 += ds * pq[1][j][0];
      e1 += ds * pq[1][j][1];
      e2 += ds * pq[1][j][2];
      e3 += ds * pq[1][j][3];
    }
    dqp[0][i][0] = scale * e0 + r * g0;
    dqp[0][i][1] = scale * e1 + r * g1;
    dqp[0][i][2] = scale * e2 + r * g2;
    dqp[0][i][3] = scale * e3 + r * g3;
  }
  __syncthreads();
  if (i < T) {   // column j = i: dk_j, dv_j over the rows in ascending order
    const int j = i;
    float k0 = 0.f, k1 = 0.f, k2 = 0.f, k3 = 0.f, v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f;
    for (int r = 0; r < T; ++r) {
      const float ds = dS[r][j], pd = Pd[r][j];
      k0 += ds * pq[0][r][0];
      k1 += ds * pq[0][r][1];
      k2 += ds * pq[0][r][2];
      k3 += ds * pq[0][r][3];
      v0 += pd * g[r][0];
      v1 += pd * g[r][1];
      v2 += pd * g[r][2];
      v3 += pd * g[r][3];
    }
    dqp[1][j][0] = scale * k0;
    dqp[1][j][1] = scale * k1;
    dqp[1][j][2] = scale * k2;
    dqp[1][j][3] = scale * k3;
    dqp[2][j][0] = v0;
    dqp[2][j][1] = v1;
    dqp[2][j][2] = v2;
    dqp[2][j][3] = v3;
  }
  __syncthreads();
  for (int it = tid; it < 3 * T; it += HS_THREADS) {   // LayerNorm(4) backward of every pooled row
    const int s = it / T, t = it - s * T;
    const float* pp = pw + s * 44;
    float c[HD], mean = 0.f;
#pragma unroll
    for (int k = 0; k < HD; ++k) {
      c[k] = pool_conv(&xr[s][0][0], HD, t, k, pp);
      mean += c[k];
    }
    mean *= 0.25f;
    float var = 0.f;
#pragma unroll
    for (int k = 0; k < HD; ++k) var += (c[k] - mean) * (c[k] - mean);
    const float rstd = rsqrtf(var * 0.25f + eps);
    float xh[HD], dxh[HD], m1 = 0.f, m2 = 0.f;
#pragma unroll
    for (int k = 0; k < HD; ++k) {
      const float d = dqp[s][t][k];
      xh[k] = (c[k] - mean) * rstd;
      dxh[k] = d * pp[36 + k];
      pgx[s][t][k] = d * xh[k];
      m1 += dxh[k];
      m2 += dxh[k] * xh[k];
    }
    m1 *= 0.25f;
    m2 *= 0.25f;
#pragma unroll
    for (int k = 0; k < HD; ++k) dc[s][t][k] = rstd * (dxh[k] - m1 - xh[k] * m2);
  }
  __syncthreads();
  float* pr = part + (long)blockIdx.x * VC_MHST_POOL_FLOATS;
  if (tid < 3 * 36) {   // conv weight gradient of (tensor s, channel k, tap)
    const int s = tid / 36, k = (tid % 36) / 9, tap = tid % 9, ky = tap / 3, kx = tap % 3;
    float acc = 0.f;
    for (int pos = 0; pos < 64; ++pos) {
      const int yy = (pos >> 3) + ky - 1, xx = (pos & 7) + kx - 1;
      if (yy < 0 || yy > 7 || xx < 0 || xx > 7) continue;
      acc += dc[s][1 + pos][k] * xr[s][1 + yy * 8 + xx][k];
    }
    pr[s * 44 + k * 9 + tap] = acc;
  } else if (tid < 3 * 36 + 12) {   // LayerNorm weight and bias gradient of (tensor s, channel k)
    const int e = tid - 3 * 36, s = e / HD, k = e % HD;
    float a = 0.f, bb = 0.f;
    for (int t = 0; t < T; ++t) {
      a += pgx[s][t][k];
      bb += dqp[s][t][k];
    }
    pr[s * 44 + 36 + k] = a;
    pr[s * 44 + 40 + k] = bb;
  }
  float ds2 = 0.f;   // d sel through the q | k | v mask: dqm . (raw q | k | v), this thread's elements in order
  for (int it = tid; it < 3 * T * HD; it += HS_THREADS) {
    const int s = it / (T * HD), t = (it / HD) % T, k = it % HD;
    float acc;
    if (t == 0) {
      acc = dc[s][0][k];
    } else {
      const int py = (t - 1) >> 3, px = (t - 1) & 7;
      const float* w = pw + s * 44 + k * 9;
      acc = 0.f;
      for (int ky = 0; ky < 3; ++ky) {
        const int yy = py - ky + 1;
        if (yy < 0 || yy > 7) continue;
        for (int kx = 0; kx < 3; ++kx) {
          const int xx = px - kx + 1;
          if (xx < 0 || xx > 7) continue;
          acc += dc[s][1 + yy * 8 + xx][k] * w[ky * 3 + kx];
        }
      }
    }
    const long gi = ((long)b * T + t) * 192 + s * DM + h * HD + k;
    ds2 += acc * QKV[gi];
    dQKV[gi] = acc * sv;
  }
  red[tid] = ds2;
  __syncthreads();
  if (tid == 0) {   // the gate, straight-through: (d sel from the MLP's mask + the two above) y (1 - y) scale
    float t = dsel_in ? dsel_in[blockIdx.x] : 0.f;
    for (int e = 0; e < HS_THREADS + T; ++e) t += red[e];
    const float yv = yg[blockIdx.x];
    dlogits[blockIdx.x] = t * yv * (1.f - yv) * gscale;
  }
}

// ------------------------------------------------------------------ dual-softmax tail
__global__ __launch_bounds__(64) void tail_fwd(int n, const float* __restrict__ lg1, const float* __restrict__ z, long ldz,
                                               const float* __restrict__ W2, const float* __restrict__ b2,
                                               const float* __restrict__ cv, const float* __restrict__ cc,
                                               float* __restrict__ p1, float* __restrict__ p2, float* __restrict__ avg,
                                               float* __restrict__ out) {
  __shared__ float av[32];
  __shared__ float l2[256];
  __shared__ float st[4];
  const int b = blockIdx.x, t = threadIdx.x;
  if (t < 32) {
    float acc = 0.f;
    for (int r = 0; r < 64; ++r) acc += z[((long)b * 64 + r) * ldz + t];
    acc *= (1.0f / 64.0f);
    av[t] = acc;
    avg[b * 32 + t] = acc;
  }
  __syncthreads();
  for (int c = t; c < n; c += 64) {
    float acc = 0.f;
    for (int kk = 0; kk < 32; ++kk) acc += W2[c * 32 + kk] * av[kk];
    l2[c] = acc + b2[c];
  }
  __syncthreads();
  if (t < 2) {   // max and sum of each softmax, serially in class order
    const float* src = t == 0 ? lg1 + (long)b * n : l2;
    float m = -INFINITY;
    for (int c = 0; c < n; ++c) m = fmaxf(m, src[c]);
    float sum = 0.f;
    for (int c = 0; c < n; ++c) sum += expf(src[c] - m);
    st[t * 2] = m;
    st[t * 2 + 1] = 1.0f / sum;
  }
  __syncthreads();
  const float a = *cv, c2 = *cc;
  for (int c = t; c < n; c += 64) {
    const float u = expf(lg1[(long)b * n + c] - st[0]) * st[1];
    const float w = expf(l2[c] - st[2]) * st[3];
    p1[(long)b * n + c] = u;
    p2[(long)b * n + c] = w;
    out[(long)b * n + c] = a * u + c2 * w;
  }
}

__global__ __launch_bounds__(64) void tail_bwd(int n, const float* __restrict__ dout, const float* __restrict__ p1,
                                               const float* __restrict__ p2, const float* __restrict__ avg,
                                               const float* __restrict__ W2, const float* __restrict__ cv,
                                               const float* __restrict__ cc, float* __restrict__ dlg1,
                                               float* __restrict__ dz, long lddz, float* __restrict__ part) {
  __shared__ float d2[256];
  __shared__ float st[2];
  const int b = blockIdx.x, t = threadIdx.x;
  const float* go = dout + (long)b * n;
  const float* u = p1 + (long)b * n;
  const float* w = p2 + (long)b * n;
  float* pr = part + (long)b * (n * 33 + 2);
  if (t < 2) {
    const float* src = t == 0 ? u : w;
    float acc = 0.f;
    for (int c = 0; c < n; ++c) acc += go[c] * src[c];
    st[t] = acc;
    pr[n * 33 + t] = acc;   // dcv, dcc
  }
  __syncthreads();
  const float a = *cv, c2 = *cc;
  for (int c = t; c < n; c += 64) {
    dlg1[(long)b * n + c] = a * u[c] * (go[c] - st[0]);
    const float d = c2 * w[c] * (go[c] - st[1]);
    d2[c] = d;
    pr[n * 32 + c] = d;
  }
  __syncthreads();
  for (int i = t; i < n * 32; i += 64) pr[i] = d2[i / 32] * avg[b * 32 + i % 32];
  if (t < 32) {
    float acc = 0.f;
    for (int c = 0; c < n; ++c) acc += d2[c] * W2[c * 32 + t];
    acc *= (1.0f / 64.0f);
    for (int r = 0; r < 64; ++r) dz[((long)b * 64 + r) * lddz + t] = acc;
  }
}

static int conv_check(const ConvShape& s, long ldi, long ldo) {
  VC_REQUIRE(s.B > 0 && s.D > 0 && s.H > 0 && s.W > 0 && s.C > 0 && s.O > 0 && s.G > 0 && s.KD > 0 && s.sd > 0);
  VC_REQUIRE(s.pd >= 0 && s.Dout > 0 && s.KS >= 1 && s.KS <= 9 && (s.KS & 1) && s.H <= 64 && s.W <= 64);
  VC_REQUIRE(s.C % s.G == 0 && s.O % s.G == 0 && s.KD <= s.D + 2 * s.pd && s.pd < s.KD);
  VC_REQUIRE(s.Dout == (s.D + 2 * s.pd - s.KD) / s.sd + 1);
  VC_REQUIRE(ldi >= s.C && ldo >= s.O);
  VC_REQUIRE_I32((long)s.B * s.D * s.H * s.W * ldi);
  VC_REQUIRE_I32((long)s.B * s.Dout * s.H * s.W * ldo);
  VC_REQUIRE_I32((long)s.O * (s.C / s.G) * s.KD * s.KS * s.KS);
  return VC_OK;
}

}  // namespace

VC_API int vc_mhst_conv_fwd(int B, int D, int H, int W, int C, int O, int G, int KD, int KS, int sd, int pd, int Dout,
                            const float* x, long ldx, const float* w, const float* bias, float* y, long ldy,
                            hipStream_t stream) {
  const ConvShape s{B, D, H, W, C, O, G, KD, KS, sd, pd, Dout};
  if (conv_check(s, ldx, ldy)) return VC_EINVAL;
  VC_REQUIRE(x && w && y);
  const long total = (long)B * Dout * H * W * O;
  hipLaunchKernelGGL(conv_fwd, dim3(vc_cdiv(total, 256)), dim3(256), 0, stream, s, total, x, ldx, w, bias, y, ldy);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

VC_API int vc_mhst_conv_dgrad(int B, int D, int H, int W, int C, int O, int G, int KD, int KS, int sd, int pd, int Dout,
                              const float* dy, long lddy, const float* w, float* dx, long lddx, float beta,
                              hipStream_t stream) {
  const ConvShape s{B, D, H, W, C, O, G, KD, KS, sd, pd, Dout};
  if (conv_check(s, lddx, lddy)) return VC_EINVAL;
  VC_REQUIRE(dy && w && dx);
  const long total = (long)B * D * H * W * C;
  hipLaunchKernelGGL(conv_dgrad, dim3(vc_cdiv(total, 256)), dim3(256), 0, stream, s, total, dy, lddy, w, dx, lddx, beta);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

VC_API int vc_mhst_conv_wgrad(int B, int D, int H, int W, int C, int O, int G, int KD, int KS, int sd, int pd, int Dout,
                              const float* x, long ldx, const float* dy, long lddy, float* dw, float* db,
                              hipStream_t stream) {
  const ConvShape s{B, D, H, W, C, O, G, KD, KS, sd, pd, Dout};
  if (conv_check(s, ldx, lddy)) return VC_EINVAL;
  VC_REQUIRE(x && dy && dw);
  VC_REQUIRE(H * W <= 64 && O / G <= WG_OG);
  const long nItems = (long)C * KD * KS * KS, nAll = nItems + (db ? O : 0);
  VC_REQUIRE_I32(nAll);
  hipLaunchKernelGGL(conv_wgrad, dim3((unsigned)nAll), dim3(64 * WG_WAVES), 0, stream, s, nItems, x, ldx, dy, lddy, dw,
                     db);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

VC_API int vc_mhst_embed_fwd(int B, const float* ph, const float* pl, const float* wh, const float* wl, const float* W,
                             const float* bias, const float* pos, const float* cls, float* xcnn, float* X0,
                             hipStream_t stream) {
  VC_REQUIRE(B > 0 && B <= 65535 && ph && pl && wh && wl && W && bias && pos && cls && xcnn && X0);
  hipLaunchKernelGGL(embed_fwd, dim3(B), dim3(256), 0, stream, ph, pl, wh, wl, W, bias, pos, cls, xcnn, X0);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

VC_API int vc_mhst_embed_bwd(int B, const float* ph, const float* pl, const float* wh, const float* wl, const float* W,
                             const float* dX0, const float* dxcnn, float* dph, float* dpl, float* part,
                             hipStream_t stream) {
  VC_REQUIRE(B > 0 && B <= 65535 && ph && pl && wh && wl && W && dX0 && dxcnn && dph && dpl && part);
  hipLaunchKernelGGL(embed_bwd, dim3(B), dim3(256), 0, stream, ph, pl, wh, wl, W, dX0, dxcnn, dph, dpl, part);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

static int gate_launch(int B, const float* X, long ldx, const float* Wg, const float* bg, const float* noise_in,
                       int train, float tau, unsigned long long seed, const unsigned long long* seed_dev, float* logits,
                       float* noise_out, float* y, float* sel, hipStream_t stream) {
  VC_REQUIRE(B > 0 && B <= (1 << 24) && ldx >= DM && tau > 0.f && (train == 0 || train == 1));
  VC_REQUIRE(X && Wg && bg && logits && y && sel);
  hipLaunchKernelGGL(gate_fwd, dim3(vc_cdiv((long)B * NH, 256)), dim3(256), 0, stream, B * NH, X, ldx, Wg, bg, noise_in,
                     train, 1.0f / tau, seed, seed_dev, logits, noise_out, y, sel);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

VC_API int vc_mhst_gate_fwd(int B, const float* X, long ldx, const float* Wg, const float* bg, const float* noise_in,
                            int train, float tau, unsigned long long seed, float* logits, float* noise_out, float* y,
                            float* sel, hipStream_t stream) {
  return gate_launch(B, X, ldx, Wg, bg, noise_in, train, tau, seed, nullptr, logits, noise_out, y, sel, stream);
}

VC_API int vc_mhst_gate_fwd_ds(int B, const float* X, long ldx, const float* Wg, const float* bg, const float* noise_in,
                               int train, float tau, const unsigned long long* seed_dev, unsigned long long site_offset,
                               float* logits, float* noise_out, float* y, float* sel, hipStream_t stream) {
  VC_REQUIRE(seed_dev);
  return gate_launch(B, X, ldx, Wg, bg, noise_in, train, tau, site_offset, seed_dev, logits, noise_out, y, sel, stream);
}

VC_API int vc_mhst_gate_bwd(int B, const float* dsel, const float* y, float scale, float* dlogits, hipStream_t stream) {
  VC_REQUIRE(B > 0 && B <= (1 << 24) && dsel && y && dlogits);
  hipLaunchKernelGGL(gate_bwd, dim3(vc_cdiv((long)B * NH, 256)), dim3(256), 0, stream, B * NH, dsel, y, scale, dlogits);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

VC_API int vc_mhst_headmask_fwd(int B, int Tn, int Wd, const float* X, const float* sel, float* Y, hipStream_t stream) {
  VC_REQUIRE(B > 0 && Tn == T && (Wd == DM || Wd == 3 * DM) && X && sel && Y);
  const long total = (long)B * T * Wd;
  VC_REQUIRE_I32(total);
  hipLaunchKernelGGL(headmask_fwd, dim3(vc_cdiv(total, 256)), dim3(256), 0, stream, total, Wd, X, sel, Y);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

VC_API int vc_mhst_headmask_bwd(int B, int Tn, int Wd, const float* dY, const float* X, const float* sel, float* dX,
                                float* dsel, float beta, hipStream_t stream) {
  VC_REQUIRE(B > 0 && B <= 65535 && Tn == T && (Wd == DM || Wd == 3 * DM) && dY && X && sel && dX && dsel);
  hipLaunchKernelGGL(headmask_bwd, dim3(B), dim3(256), 0, stream, Wd, dY, X, sel, dX, dsel, beta);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

VC_API int vc_mhst_pool_fwd(int B, const float* X, const float* pw, float eps, float* Y, hipStream_t stream) {
  VC_REQUIRE(B > 0 && B <= 65535 && eps > 0.f && X && pw && Y);
  const long total = (long)B * T * 3 * NH;
  hipLaunchKernelGGL(pool_fwd, dim3(vc_cdiv(total, 256)), dim3(256), 0, stream, total, X, pw, eps, Y);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

VC_API int vc_mhst_pool_bwd(int B, const float* X, const float* pw, float eps, const float* dY, float* dX, float* part,
                            hipStream_t stream) {
  VC_REQUIRE(B > 0 && B <= 65535 && eps > 0.f && X && pw && dY && dX && part);
  hipLaunchKernelGGL(pool_bwd, dim3(B, 3), dim3(256), 0, stream, X, pw, eps, dY, dX, part);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

static int attn_launch(int B, const float* QKV, float scale, float p, unsigned long long seed,
                       const unsigned long long* seed_dev, unsigned char* mask, float* O, hipStream_t stream) {
  VC_REQUIRE(B > 0 && p >= 0.f && p < 1.f && QKV && O && (mask || p == 0.f));
  VC_REQUIRE_I32((long)B * NH * T * T);
  const int total = B * NH * T;
  hipLaunchKernelGGL(attn_fwd, dim3(vc_cdiv(total, 256)), dim3(256), 0, stream, total, QKV, scale, p, seed, seed_dev,
                     mask, O);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

VC_API int vc_mhst_attn_fwd(int B, const float* QKV, float scale, float p, unsigned long long seed, unsigned char* mask,
                            float* O, hipStream_t stream) {
  return attn_launch(B, QKV, scale, p, seed, nullptr, mask, O, stream);
}

VC_API int vc_mhst_attn_fwd_ds(int B, const float* QKV, float scale, float p, const unsigned long long* seed_dev,
                               unsigned long long site_offset, unsigned char* mask, float* O, hipStream_t stream) {
  VC_REQUIRE(seed_dev);
  return attn_launch(B, QKV, scale, p, site_offset, seed_dev, mask, O, stream);
}

VC_API int vc_mhst_attn_bwd(int B, const float* QKV, float scale, float p, const unsigned char* mask, const float* dO,
                            float* dQKV, hipStream_t stream) {
  VC_REQUIRE(B > 0 && p >= 0.f && p < 1.f && QKV && dO && dQKV && (mask || p == 0.f));
  VC_REQUIRE_I32((long)B * NH * T * T);
  hipLaunchKernelGGL(attn_bwd, dim3(B * NH), dim3(128), 0, stream, QKV, scale, p, mask, dO, dQKV);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

VC_API int vc_mhst_tail_fwd(int B, int ncls, const float* lg1, const float* z, long ldz, const float* W2,
                            const float* b2, const float* cv, const float* cc, float* p1, float* p2, float* avg,
                            float* out, hipStream_t stream) {
  VC_REQUIRE(B > 0 && B <= 65535 && ncls >= 1 && ncls <= 256 && ldz >= 32);
  VC_REQUIRE(lg1 && z && W2 && b2 && cv && cc && p1 && p2 && avg && out);
  hipLaunchKernelGGL(tail_fwd, dim3(B), dim3(64), 0, stream, ncls, lg1, z, ldz, W2, b2, cv, cc, p1, p2, avg, out);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

VC_API int vc_mhst_tail_bwd(int B, int ncls, const float* dout, const float* p1, const float* p2, const float* avg,
                            const float* W2, const float* cv, const float* cc, float* dlg1, float* dz, long lddz,
                            float* part, hipStream_t stream) {
  VC_REQUIRE(B > 0 && B <= 65535 && ncls >= 1 && ncls <= 256 && lddz >= 32);
  VC_REQUIRE(dout && p1 && p2 && avg && W2 && cv && cc && dlg1 && dz && part);
  hipLaunchKernelGGL(tail_bwd, dim3(B), dim3(64), 0, stream, ncls, dout, p1, p2, avg, W2, cv, cc, dlg1, dz, lddz, part);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

static int conv3_check(int B, int D, const float* a, long lda, const void* b, long ldb) {
  VC_REQUIRE(B > 0 && D > 0 && a && b && lda >= C3 && ldb >= C3);
  VC_REQUIRE((long)B * D <= (1L << 30));
  VC_REQUIRE_I32((long)B * D * 64 * std::max(lda, ldb));
  return VC_OK;
}

VC_API int vc_mhst_conv3_fwd(int B, int D, const float* x, long ldx, const float* w, const float* bias, float* y,
                             long ldy, hipStream_t stream) {
  if (conv3_check(B, D, x, ldx, y, ldy)) return VC_EINVAL;
  VC_REQUIRE(w && ldx % 4 == 0 && ((uintptr_t)x & 15) == 0);
  hipLaunchKernelGGL(conv3_mfma<0>, dim3(B * D), dim3(256), 0, stream, D, x, ldx, w, bias, y, ldy, 0.f);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

VC_API int vc_mhst_conv3_dgrad(int B, int D, const float* dy, long lddy, const float* w, float* dx, long lddx,
                               float beta, hipStream_t stream) {
  if (conv3_check(B, D, dy, lddy, dx, lddx)) return VC_EINVAL;
  VC_REQUIRE(w && lddy % 4 == 0 && ((uintptr_t)dy & 15) == 0);
  hipLaunchKernelGGL(conv3_mfma<1>, dim3(B * D), dim3(256), 0, stream, D, dy, lddy, w, (const float*)nullptr, dx, lddx,
                     beta);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

VC_API int vc_mhst_conv3_wgrad_ws_floats(int B, int D) {
  if (B <= 0 || D <= 0 || (long)B * D > (1L << 30)) return -1;
  return (int)std::min<long>(VC_MHST_CONV3_WAVES, (long)B * D) * C3_W;
}

VC_API int vc_mhst_conv3_wgrad(int B, int D, const float* x, long ldx, const float* dy, long lddy, float* dw, float* ws,
                               long ws_floats, hipStream_t stream) {
  if (conv3_check(B, D, x, ldx, dy, lddy)) return VC_EINVAL;
  const int planes = B * D, nb = std::min(VC_MHST_CONV3_WAVES, planes);
  VC_REQUIRE(dw && ws && ws_floats >= (long)nb * C3_W);
  hipLaunchKernelGGL(conv3_wgrad_mfma, dim3(nb), dim3(64), 0, stream, planes, D, x, ldx, dy, lddy, ws);
  VC_CHECK_LAUNCH();
  return launch_sum_rows(nb, C3_W, ws, C3_W, 0, dw, 0.f, stream);
}

static int hsattn_launch(int B, const float* X, long ldx, const float* Wg, const float* bg, const float* noise_in,
                         int train, float tau, unsigned long long seed_gate, unsigned long long seed_prob,
                         const unsigned long long* seed_dev, const float* QKV, const float* pw, float eps, float scale,
                         float p, unsigned char* mask, float* logits, float* noise_out, float* y, float* sel, float* AM,
                         hipStream_t stream) {
  VC_REQUIRE(B > 0 && ldx >= DM && tau > 0.f && (train == 0 || train == 1) && eps > 0.f && p >= 0.f && p < 1.f);
  VC_REQUIRE(X && Wg && bg && QKV && pw && logits && y && sel && AM && (mask || p == 0.f));
  VC_REQUIRE_I32((long)B * NH * T * T);
  hipLaunchKernelGGL(hsattn_fwd, dim3(B * NH), dim3(HS_THREADS), 0, stream, X, ldx, Wg, bg, noise_in, train, 1.0f / tau,
                     seed_gate, seed_prob, seed_dev, QKV, pw, eps, scale, p, mask, logits, noise_out, y, sel, AM);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

VC_API int vc_mhst_hsattn_fwd(int B, const float* X, long ldx, const float* Wg, const float* bg, const float* noise_in,
                              int train, float tau, unsigned long long seed_gate, unsigned long long seed_prob,
                              const float* QKV, const float* pw, float eps, float scale, float p, unsigned char* mask,
                              float* logits, float* noise_out, float* y, float* sel, float* AM, hipStream_t stream) {
  return hsattn_launch(B, X, ldx, Wg, bg, noise_in, train, tau, seed_gate, seed_prob, nullptr, QKV, pw, eps, scale, p,
                       mask, logits, noise_out, y, sel, AM, stream);
}

VC_API int vc_mhst_hsattn_fwd_ds(int B, const float* X, long ldx, const float* Wg, const float* bg,
                                 const float* noise_in, int train, float tau, const unsigned long long* seed_dev,
                                 unsigned long long gate_offset, unsigned long long prob_offset, const float* QKV,
                                 const float* pw, float eps, float scale, float p, unsigned char* mask, float* logits,
                                 float* noise_out, float* y, float* sel, float* AM, hipStream_t stream) {
  VC_REQUIRE(seed_dev);
  return hsattn_launch(B, X, ldx, Wg, bg, noise_in, train, tau, gate_offset, prob_offset, seed_dev, QKV, pw, eps, scale,
                       p, mask, logits, noise_out, y, sel, AM, stream);
}

VC_API int vc_mhst_hsattn_bwd(int B, const float* QKV, const float* sel, const float* y, const float* pw, float eps,
                              float scale, float p, const unsigned char* mask, const float* dAM, const float* dsel_in,
                              float gscale, float* dQKV, float* part, float* dlogits, hipStream_t stream) {
  VC_REQUIRE(B > 0 && eps > 0.f && p >= 0.f && p < 1.f);
  VC_REQUIRE(QKV && sel && y && pw && dAM && dQKV && part && dlogits && (mask || p == 0.f));
  VC_REQUIRE_I32((long)B * NH * T * T);
  hipLaunchKernelGGL(hsattn_bwd, dim3(B * NH), dim3(HS_THREADS), 0, stream, QKV, sel, y, pw, eps, scale, p, mask, dAM,
                     dsel_in, gscale, dQKV, part, dlogits);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

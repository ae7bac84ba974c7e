// The front of MHST's HSI encoder as implicit GEMMs on v_mfma_f32_16x16x4_f32 (A: row = lane & 15, k = lane >> 4;
// B: col = lane & 15, k = lane >> 4; D: col = lane & 15, row = (lane >> 4) * 4 + r): the strided first convolution
// (vc_mhst_conv1_*) and the four spectral convolutions as ONE convolution (vc_mhst_sconv_*).  Formulas and the
// alignment contract: include/vitcnn.h; the formulation and what it costs: DESIGN.md section 28.
// Exact fp32: an MFMA is a k-ordered fmaf chain.  No atomics; every partial is summed in a fixed order.
//
//   conv1 fwd    M = (b, e, position)  N = 16  K = (kh, kw, kd padded to 12) = 108: 27 MFMA steps whose lane row kq
//                stands for kd = 4 j + kq, so a lane's LDS address is its own base plus a compile-time constant
//   conv1 wgrad  M = 16 outputs  N = 99 taps (+ a column of ones: the bias gradient) in 7 tiles  K = (b, e, position)
//   sconv fwd    M = (b, e, position)  N = 16 (the four convolutions' columns)  K = 11 depth offsets x 16 channels
//   sconv dgrad  the same kernel, operand roles swapped and the offsets mirrored
//   sconv wgrad  M = 16 columns  N = 16 channels, one accumulator per depth offset  K = (b, e, position)
// The inputs a block needs sit in LDS (zero-padded 10 x 10 planes for conv1, so the spatial and spectral halo is never
// read from global memory outside the cube; whole 64 x 16 planes for sconv), read once per block.
#include "common.h"

namespace {

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// ------------------------------------------------------------------ conv1
constexpr int C1_E = VC_MHST_CONV1_CHUNK;        // output depths per forward block
constexpr int C1_PLANES = 3 * (C1_E - 1) + 12;   // its input planes, + the one the zero tap kd = 11 addresses
constexpr int C1_PL = 100;                       // a zero-padded 10 x 10 plane
constexpr int C1_TAPS = 99, C1_STEPS = 27;
constexpr int C1_ROW = 1600;                     // a weight-gradient partial: dw [16][99] | db [16]

// xs[pl][hh + 1][ww + 1] = x[b, d0 + pl, hh, ww], 0 outside the cube
__device__ __forceinline__ void c1_stage(float* xs, int nplanes, const float* __restrict__ x, int b, int l1, int d0,
                                         int tid, int nthreads) {
  for (int i = tid; i < nplanes * C1_PL; i += nthreads) {
    const int pl = i / C1_PL, r = i - pl * C1_PL, hr = r / 10, hh = hr - 1, ww = r - hr * 10 - 1, d = d0 + pl;
    const bool in = hh >= 0 && hh < 8 && ww >= 0 && ww < 8 && d >= 0 && d < l1;
    xs[i] = in ? x[((long)b * l1 + d) * 64 + hh * 8 + ww] : 0.f;
  }
}

// A block owns (sample, C1_E output depths); a wave 16 positions of each of them: C1_E accumulators share each B value.
__global__ __launch_bounds__(256) void conv1_fwd_k(int l1, int D1, int nchunks, const float* __restrict__ x,
                                                   const float* __restrict__ w, const float* __restrict__ bias,
                                                   float* __restrict__ y, long ldy) {
  __shared__ float xs[C1_PLANES * C1_PL];
  __shared__ float wl[C1_STEPS * 64];
  const int b = blockIdx.x / nchunks, e0 = (blockIdx.x - b * nchunks) * C1_E;
  // wl[(i 4 + kq) 16 + o] = w[o][kd = 4 j + kq][kh][kw] with i = (kh 3 + kw) 3 + j; 0 at kd = 11
  for (int i = threadIdx.x; i < C1_STEPS * 64; i += 256) {
    const int o = i & 15, kq = (i >> 4) & 3, st = i >> 6, j = st % 3, khw = st / 3, kd = 4 * j + kq;
    wl[i] = kd < 11 ? w[o * C1_TAPS + kd * 9 + khw] : 0.f;
  }
  c1_stage(xs, C1_PLANES, x, b, l1, 3 * e0 - 5, threadIdx.x, 256);
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, m = lane & 15, kq = lane >> 4;
  const int pos = wave * 16 + m;
  const float* xa = xs + kq * C1_PL + (pos >> 3) * 10 + (pos & 7);
  const float* wb = wl + kq * 16 + m;
  f32x4 acc[C1_E];
#pragma unroll
  for (int t = 0; t < C1_E; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int st = 0; st < C1_STEPS; ++st) {
    const int j = st % 3, khw = st / 3, off = j * 4 * C1_PL + (khw / 3) * 10 + khw % 3;
    const float bv = wb[st * 64];
    const bool pad = j == 2 && kq == 3;   // kd = 11: both operands 0, whatever the plane holds
#pragma unroll
    for (int t = 0; t < C1_E; ++t) {
      const float a = xa[t * 3 * C1_PL + off];
      acc[t] = mfma4(pad ? 0.f : a, bv, acc[t]);
    }
  }
  const float bs = bias ? bias[m] : 0.f;
#pragma unroll
  for (int t = 0; t < C1_E; ++t) {
    if (e0 + t >= D1) break;
#pragma unroll
    for (int r = 0; r < 4; ++r)
      y[(((long)b * D1 + e0 + t) * 64 + wave * 16 + kq * 4 + r) * ldy + m] = acc[t][r] + bs;
  }
}

// One wave per block walks the (sample, output depth) planes blockIdx.x, + gridDim.x, ... in order: the plane's 11 input
// planes go to LDS once, then 16 k-steps of 4 positions feed 7 tap tiles.  Tap 99 is a column of ones, so its
// accumulator is the bias gradient.  The wave's partial [dw 16 x 99 | db 16] goes to part; c1_sum adds them in order.
__global__ __launch_bounds__(64) void conv1_wgrad_k(int planes, int l1, int D1, const float* __restrict__ x,
                                                    const float* __restrict__ dy, long lddy,
                                                    float* __restrict__ part) {
  __shared__ float xs[11 * C1_PL];
  const int lane = threadIdx.x, m = lane & 15, kq = lane >> 4;
  int toff[7];
#pragma unroll
  for (int T = 0; T < 7; ++T) {
    const int tap = T * 16 + m, kd = tap / 9, r = tap - kd * 9;
    toff[T] = tap < C1_TAPS ? kd * C1_PL + (r / 3) * 10 + r % 3 + kq : 0;
  }
  f32x4 acc[7];
#pragma unroll
  for (int T = 0; T < 7; ++T) acc[T] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int plane = blockIdx.x; plane < planes; plane += gridDim.x) {
    const int b = plane / D1, e = plane - b * D1;
    __syncthreads();   // the previous plane's reads are done
    c1_stage(xs, 11, x, b, l1, 3 * e - 5, lane, 64);
    float a[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) a[s] = dy[((long)plane * 64 + 4 * s + kq) * lddy + m];
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const int po = (s >> 1) * 10 + (s & 1) * 4;   // positions 4 s .. 4 s + 3 share an image row
#pragma unroll
      for (int T = 0; T < 7; ++T) {
        float bv = xs[toff[T] + po];
        if (T == 6) bv = m == 3 ? 1.f : (m > 3 ? 0.f : bv);
        acc[T] = mfma4(a[s], bv, acc[T]);
      }
    }
  }
  float* pr = part + (long)blockIdx.x * C1_ROW;
#pragma unroll
  for (int T = 0; T < 7; ++T) {
    const int tap = T * 16 + m;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int o = kq * 4 + r;
      if (tap < C1_TAPS) pr[o * C1_TAPS + tap] = acc[T][r];
      if (tap == C1_TAPS) pr[16 * C1_TAPS + o] = acc[T][r];
    }
  }
}

// sum_{p < P} part[p stride + c] for the block's 16 columns, 16 partial lanes each, combined in a fixed order
// (sum_rows_kernel's scheme); the result is valid where threadIdx.x < 16
__device__ __forceinline__ float part_sum16(int P, const float* __restrict__ part, long stride, int c, bool ok) {
  __shared__ float sh[16][17];
  const int cl = threadIdx.x & 15, pl = threadIdx.x >> 4;
  float s = 0.f;
  if (ok) {
#pragma unroll 4
    for (int p = pl; p < P; p += 16) s += part[(long)p * stride + c];
  }
  sh[pl][cl] = s;
  __syncthreads();
  float v = 0.f;
  if (pl == 0) {
#pragma unroll
    for (int i = 0; i < 16; ++i) v += sh[i][cl];
  }
  return v;
}

__global__ __launch_bounds__(256) void c1_sum(int P, const float* __restrict__ part, float* __restrict__ dw,
                                              float* __restrict__ db) {
  const int c = blockIdx.x * 16 + (threadIdx.x & 15);   // C1_ROW is a multiple of 16
  const float v = part_sum16(P, part, C1_ROW, c, true);
  if (threadIdx.x >= 16) return;
  if (c < 16 * C1_TAPS)
    dw[c] = v;
  else if (db)
    db[c - 16 * C1_TAPS] = v;
}

// ------------------------------------------------------------------ sconv
constexpr int SC_E = VC_MHST_SCONV_CHUNK;     // depths per block: one per wave
constexpr int SC_T = 11, SC_R = 5;            // depth offsets -5 .. 5
constexpr int SC_PLANES = SC_E + 2 * SC_R;
constexpr int SC_W = SC_T * 256;              // the padded weight [t][k][n]
constexpr int SC_ROW = SC_W + 16;             // a weight-gradient partial: [t][n][c] | db [16]

struct SW {
  const float* p[4];
};
struct SWOut {
  float* p[4];
};

// the padded weight's entry (offset tt - 5, channel c, column n): w_i[j][c][t + r_i] with n = 4 i + j, 0 where |t| > r_i
__device__ __forceinline__ int sc_src(int tt, int c, int n, int& i) {
  i = n >> 2;
  const int r = i == 3 ? 5 : i, t = tt - SC_R;
  if (t < -r || t > r) return -1;
  return ((n & 3) * 16 + c) * (2 * r + 1) + t + r;
}

// MODE 0: the forward, k = channel, n = column, source depth e + t.  MODE 1: the data gradient, k = column, n = channel,
// source depth e - t.  A block owns (sample, SC_E depths): their SC_PLANES source planes sit in LDS as they lie
// [plane][position][16]; a wave owns one depth, its 64 positions in 4 tiles whose accumulators share each B value.  A
// lane reads the 4 values 4 kq .. 4 kq + 3 of its row as one float4 and feeds 4 MFMAs (conv3_mfma's inner step).
template <int MODE>
__global__ __launch_bounds__(256) void sconv_k(int D, int nchunks, const float* __restrict__ in, long ldi, SW w, SW bias,
                                               float* __restrict__ out, long ldo, float beta) {
  __shared__ f32x4 xs[SC_PLANES * 64 * 4];
  __shared__ float wl[SC_W];
  const int b = blockIdx.x / nchunks, e0 = (blockIdx.x - b * nchunks) * SC_E;
  for (int i = threadIdx.x; i < SC_W; i += 256) {
    const int tt = i >> 8, k = (i >> 4) & 15, n = i & 15;
    int wi;
    const int src = MODE == 0 ? sc_src(tt, k, n, wi) : sc_src(tt, n, k, wi);
    wl[i] = src >= 0 ? w.p[wi][src] : 0.f;
  }
  for (int i = threadIdx.x; i < SC_PLANES * 256; i += 256) {
    const int pl = i >> 8, d = e0 - SC_R + pl;
    if (d >= 0 && d < D)   // a plane outside the cube is never read
      xs[i] = *reinterpret_cast<const f32x4*>(in + (((long)b * D + d) * 64 + ((i >> 2) & 63)) * ldi + 4 * (i & 3));
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, m = lane & 15, kq = lane >> 4;
  const int e = e0 + wave;
  if (e >= D) return;   // wave-uniform, after the only barrier
  f32x4 acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int tt = 0; tt < SC_T; ++tt) {
    const int d = MODE == 0 ? e + tt - SC_R : e - tt + SC_R;
    if (d < 0 || d >= D) continue;   // wave-uniform
    const f32x4* xp = xs + ((d - e0 + SC_R) * 64 + m) * 4 + kq;
    f32x4 a[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) a[q] = xp[q * 64];
    const float* wt = wl + (tt * 16 + 4 * kq) * 16 + m;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float bv = wt[j * 16];
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] = mfma4(a[q][j], bv, acc[q]);
    }
  }
  float bs = 0.f;
  if (MODE == 0 && bias.p[0]) bs = bias.p[m >> 2][m & 3];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float* o = out + (((long)b * D + e) * 64 + q * 16 + kq * 4 + r) * ldo + m;
      *o = (beta != 0.f ? beta * *o : 0.f) + acc[q][r] + bs;
    }
}

// A block walks the (sample, SC_E depths) items blockIdx.x, + gridDim.x, ... in order: the item's x planes go to LDS, a
// wave owns one depth's dy plane (16 k-steps of 4 rows) with one accumulator per depth offset; a lane also adds up the dy
// values it feeds (the bias gradient).  Then the 4 waves are summed in wave order through LDS and the block's partial
// [t][n][c] | db [16] goes to part; sc_sum adds the blocks in order and scatters the real entries.
__global__ __launch_bounds__(256) void sconv_wgrad_k(int items, int D, int nchunks, const float* __restrict__ x,
                                                     long ldx, const float* __restrict__ dy, long lddy,
                                                     float* __restrict__ part) {
  __shared__ f32x4 xs4[SC_PLANES * 64 * 4];
  static_assert(SC_PLANES * 64 * 16 >= 4 * SC_ROW, "the waves' partials reuse the planes' LDS");
  float* xs = reinterpret_cast<float*>(xs4);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, m = lane & 15, kq = lane >> 4;
  f32x4 acc[SC_T];
#pragma unroll
  for (int tt = 0; tt < SC_T; ++tt) acc[tt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float dbs = 0.f;
  for (int item = blockIdx.x; item < items; item += gridDim.x) {   // block-uniform
    const int b = item / nchunks, e0 = (item - b * nchunks) * SC_E;
    __syncthreads();   // the previous item's reads are done
    for (int i = threadIdx.x; i < SC_PLANES * 256; i += 256) {
      const int pl = i >> 8, d = e0 - SC_R + pl;
      if (d >= 0 && d < D)
        xs4[i] = *reinterpret_cast<const f32x4*>(x + (((long)b * D + d) * 64 + ((i >> 2) & 63)) * ldx + 4 * (i & 3));
    }
    const int e = e0 + wave;
    float a[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) a[s] = e < D ? dy[(((long)b * D + e) * 64 + 4 * s + kq) * lddy + m] : 0.f;
    __syncthreads();
    if (e < D) {   // wave-uniform
#pragma unroll
      for (int s = 0; s < 16; ++s) dbs += a[s];
#pragma unroll
      for (int tt = 0; tt < SC_T; ++tt) {
        const int d = e + tt - SC_R;
        if (d < 0 || d >= D) continue;   // wave-uniform
        const float* xp = xs + ((d - e0 + SC_R) * 64 + kq) * 16 + m;
#pragma unroll
        for (int s = 0; s < 16; ++s) acc[tt] = mfma4(a[s], xp[s * 64], acc[tt]);
      }
    }
  }
  dbs += __shfl_xor(dbs, 16, 64);
  dbs += __shfl_xor(dbs, 32, 64);
  __syncthreads();
  float* red = xs + wave * SC_ROW;
#pragma unroll
  for (int tt = 0; tt < SC_T; ++tt)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[tt * 256 + (kq * 4 + r) * 16 + m] = acc[tt][r];
  if (kq == 0) red[SC_W + m] = dbs;
  __syncthreads();
  float* pr = part + (long)blockIdx.x * SC_ROW;
  for (int i = threadIdx.x; i < SC_ROW; i += 256)
    pr[i] = ((xs[i] + xs[SC_ROW + i]) + xs[2 * SC_ROW + i]) + xs[3 * SC_ROW + i];
}

__global__ __launch_bounds__(256) void sc_sum(int P, const float* __restrict__ part, SWOut dw, SWOut db) {
  const int c = blockIdx.x * 16 + (threadIdx.x & 15);   // SC_ROW is a multiple of 16
  int wi = 0, dst = -1;
  if (c < SC_W)
    dst = sc_src(c >> 8, c & 15, (c >> 4) & 15, wi);   // the partial is [t][n][c]
  const bool isdb = c >= SC_W && db.p[0];
  const float v = part_sum16(P, part, SC_ROW, c, dst >= 0 || isdb);
  if (threadIdx.x >= 16) return;
  if (dst >= 0) dw.p[wi][dst] = v;
  if (isdb) db.p[(c - SC_W) >> 2][(c - SC_W) & 3] = v;
}

// ------------------------------------------------------------------ host checks
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
bool ld_ok(long ld) { return ld >= 16 && (ld & 3) == 0; }

int c1_waves(int B, int D1) { return (int)std::min<long>(VC_MHST_CONV1_WAVES, (long)B * D1); }
int sc_blocks(int B, int D) { return (int)std::min<long>(VC_MHST_SCONV_BLOCKS, (long)B * vc_cdiv(D, SC_E)); }

bool c1_shape(int B, int l1) {
  return B >= 1 && l1 >= 1 && (long)B * l1 * 64 < (1L << 31) && (long)B * vc_cdiv((l1 + 2) / 3, C1_E) < (1L << 31);
}
// rows of at least 16 floats index in 32 bits only below 2^27 rows
bool sc_shape(int B, int D) { return B >= 1 && D >= 1 && (long)B * D * 64 < (1L << 27); }

}  // namespace

VC_API int vc_mhst_conv1_ws_floats(int B, int l1) {
  if (!c1_shape(B, l1)) return -1;
  return c1_waves(B, (l1 + 2) / 3) * C1_ROW;
}

VC_API int vc_mhst_conv1_fwd(int B, int l1, const float* x, const float* w, const float* bias, float* y, long ldy,
                             float* ws, long ws_floats, hipStream_t stream) {
  VC_REQUIRE(c1_shape(B, l1) && ld_ok(ldy));
  const int D1 = (l1 + 2) / 3, nchunks = vc_cdiv(D1, C1_E);
  VC_REQUIRE_I32((long)B * D1 * 64 * ldy);
  VC_REQUIRE(x && w && y && ws && ws_floats >= vc_mhst_conv1_ws_floats(B, l1));
  VC_REQUIRE(aligned16(x) && aligned16(y) && aligned16(ws));
  hipLaunchKernelGGL(conv1_fwd_k, dim3(B * nchunks), dim3(256), 0, stream, l1, D1, nchunks, x, w, bias, y, ldy);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

VC_API int vc_mhst_conv1_wgrad(int B, int l1, const float* x, const float* dy, long lddy, float* dw, float* db,
                               float* ws, long ws_floats, hipStream_t stream) {
  VC_REQUIRE(c1_shape(B, l1) && ld_ok(lddy));
  const int D1 = (l1 + 2) / 3, nw = c1_waves(B, D1);
  VC_REQUIRE_I32((long)B * D1 * 64 * lddy);
  VC_REQUIRE(x && dy && dw && ws && ws_floats >= vc_mhst_conv1_ws_floats(B, l1));
  VC_REQUIRE(aligned16(x) && aligned16(dy) && aligned16(ws));
  hipLaunchKernelGGL(conv1_wgrad_k, dim3(nw), dim3(64), 0, stream, B * D1, l1, D1, x, dy, lddy, ws);
  VC_CHECK_LAUNCH();
  hipLaunchKernelGGL(c1_sum, dim3(C1_ROW / 16), dim3(256), 0, stream, nw, ws, dw, db);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

VC_API int vc_mhst_sconv_ws_floats(int B, int D) {
  if (!sc_shape(B, D)) return -1;
  return sc_blocks(B, D) * SC_ROW;
}

// the checks the three directions share; a / b: the two row operands and their leading dimensions
static int sconv_check(int B, int D, const void* a, long lda, const void* b, long ldb, const void* ws, long ws_floats) {
  VC_REQUIRE(sc_shape(B, D) && ld_ok(lda) && ld_ok(ldb));
  VC_REQUIRE_I32((long)B * D * 64 * std::max(lda, ldb));
  VC_REQUIRE(a && b && ws && ws_floats >= vc_mhst_sconv_ws_floats(B, D));
  VC_REQUIRE(aligned16(a) && aligned16(b) && aligned16(ws));
  return VC_OK;
}

VC_API int vc_mhst_sconv_fwd(int B, int D, const float* x, long ldx, const float* w1, const float* w2, const float* w3,
                             const float* w4, const float* b1, const float* b2, const float* b3, const float* b4,
                             float* y, long ldy, float* ws, long ws_floats, hipStream_t stream) {
  if (sconv_check(B, D, x, ldx, y, ldy, ws, ws_floats)) return VC_EINVAL;
  VC_REQUIRE(w1 && w2 && w3 && w4);
  const int nb = (b1 != nullptr) + (b2 != nullptr) + (b3 != nullptr) + (b4 != nullptr);
  VC_REQUIRE(nb == 0 || nb == 4);
  const int nchunks = vc_cdiv(D, SC_E);
  hipLaunchKernelGGL(sconv_k<0>, dim3(B * nchunks), dim3(256), 0, stream, D, nchunks, x, ldx, SW{{w1, w2, w3, w4}},
                     SW{{b1, b2, b3, b4}}, y, ldy, 0.f);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

VC_API int vc_mhst_sconv_dgrad(int B, int D, const float* dy, long lddy, const float* w1, const float* w2,
                               const float* w3, const float* w4, float* dx, long lddx, float beta, float* ws,
                               long ws_floats, hipStream_t stream) {
  if (sconv_check(B, D, dy, lddy, dx, lddx, ws, ws_floats)) return VC_EINVAL;
  VC_REQUIRE(w1 && w2 && w3 && w4);
  const int nchunks = vc_cdiv(D, SC_E);
  hipLaunchKernelGGL(sconv_k<1>, dim3(B * nchunks), dim3(256), 0, stream, D, nchunks, dy, lddy, SW{{w1, w2, w3, w4}},
                     SW{{nullptr, nullptr, nullptr, nullptr}}, dx, lddx, beta);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

VC_API int vc_mhst_sconv_wgrad(int B, int D, const float* x, long ldx, const float* dy, long lddy, float* dw1,
                               float* dw2, float* dw3, float* dw4, float* db1, float* db2, float* db3, float* db4,
                               float* ws, long ws_floats, hipStream_t stream) {
  if (sconv_check(B, D, x, ldx, dy, lddy, ws, ws_floats)) return VC_EINVAL;
  VC_REQUIRE(dw1 && dw2 && dw3 && dw4);
  const int nb = (db1 != nullptr) + (db2 != nullptr) + (db3 != nullptr) + (db4 != nullptr);
  VC_REQUIRE(nb == 0 || nb == 4);
  const int nchunks = vc_cdiv(D, SC_E), blocks = sc_blocks(B, D);
  hipLaunchKernelGGL(sconv_wgrad_k, dim3(blocks), dim3(256), 0, stream, B * nchunks, D, nchunks, x, ldx, dy, lddy, ws);
  VC_CHECK_LAUNCH();
  hipLaunchKernelGGL(sc_sum, dim3(SC_ROW / 16), dim3(256), 0, stream, blocks, ws, SWOut{{dw1, dw2, dw3, dw4}},
                     SWOut{{db1, db2, db3, db4}});
  VC_CHECK_LAUNCH();
  return VC_OK;
}

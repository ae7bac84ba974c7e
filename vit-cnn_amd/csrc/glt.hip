// GLT-Net (the global-local transformer of the comparison table; three scales P, 2P, 3P of one patch) -- the kernels
// that the model needs beyond the shared ones.  Formulas: include/vitcnn.h, "GLT-Net".  All fp32, no float atomics;
// every reduction runs in a fixed order, so two runs are bit-identical.
//
//   crops    : one NCHW 3P patch -> the three centre crops as channels-last rows (conv inputs and MSE targets)
//   fuse     : x1 xishu1 + x2 xishu2 at three scales -> the three spatial Linears -> SA-GDR (mean / max over the three,
//              7x7 conv, sigmoid) -> tokens + position rows + cls row; one block per sample, the sample's fused maps
//              (3.5 P^2 x 64 floats, 56 KB at P = 8) in LDS.  The embedding matrices (14,336 floats at P = 8) are NOT
//              staged: every wave reads one W[j][p] at a time as a wave-uniform (scalar-cache) load, and 56 + 56 KB
//              would leave one block per CU where the maps alone leave two.
//   upconv   : nearest upsample by s folded into the 3x3 implicit GEMM (conv_tap.hip's structure: tap-major K, 128 x 128
//              tiles on v_mfma_f32_32x32x2_f32, split-K with a fixed-order combine): the gathered row of tap (dy, dx) at
//              output (y, x) is input pixel (floor((y + dy - 1) / s), floor((x + dx - 1) / s)); the upsampled tensor is
//              never written.  The data gradient walks K = (s x s replicas) x 9 taps x O, so the replicas are summed
//              in the accumulator.  Where O, C and the leading dimensions are multiples of 4 (the 144-band branch) the
//              same GEMMs run on 64 x 64 tiles of the LDS-DMA pipeline (upconv_pipe), the upsample in the DMA offsets.
//   sigmse   : sigmoid + squared error against a crop, block partials in fp64, combined by the last-arriving block in
//              block order
//   tail     : average pool, 1x1 conv to the classes, softmax, mixed with the transformer head's logits
#include "common.h"
#include "mfma_tiles.h"

#include <algorithm>

namespace {

// ------------------------------------------------------------------ crops
// rows r of the three outputs back to back: [B, P^2], [B, 4 P^2], [B, 9 P^2]; thread per (row, column of ld)
__global__ __launch_bounds__(256) void crops_kernel(int B, int C, int P, int ld, long total,
                                                    const float* __restrict__ x, float* __restrict__ r1,
                                                    float* __restrict__ r2, float* __restrict__ r3) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int c = (int)(e % ld);
  long row = e / ld;
  const long n1 = (long)B * P * P, n2 = 4 * n1;
  int k, side, off;
  float* dst;
  if (row < n1) {
    k = 1; side = P; off = P; dst = r1;
  } else if (row < n1 + n2) {
    k = 2; side = 2 * P; off = P / 2; dst = r2; row -= n1;
  } else {
    k = 3; side = 3 * P; off = 0; dst = r3; row -= n1 + n2;
  }
  (void)k;
  const int b = (int)(row / (side * side));
  const int r = (int)(row - (long)b * side * side);
  const int i = r / side, j = r - i * side;
  const int S = 3 * P;
  dst[row * ld + c] = c < C ? x[(((long)b * C + c) * S + (i + off)) * S + (j + off)] : 0.f;
}

// ------------------------------------------------------------------ fusion + embedding + SA-GDR
constexpr int FD = 64;          // channels of the fused maps = token width
constexpr int FP_MAX = 8;       // largest model patch side
constexpr int FNP_MAX = FP_MAX * FP_MAX;
constexpr int FROWS_MAX = FNP_MAX / 4 + FNP_MAX + 9 * FNP_MAX / 4;   // 224 pooled positions over the three scales

struct FuseArgs {
  int B, P;
  const float* pa[3];
  const float* pb[3];
  const float* W[3];
  const float* bias[3];
  const float *xs1, *xs2, *w7, *pos, *cls;
  // forward outputs; backward inputs
  float *xcnn, *X0, *e;
  const float *dX0, *dxcnn;
  float* dpa[3];
  float* dpb[3];
  float* part;
};

__device__ __forceinline__ float sigmoid_exact(float x) { return 1.0f / (1.0f + expf(-x)); }

__global__ __launch_bounds__(256) void fuse_fwd(FuseArgs a) {
  __shared__ __attribute__((aligned(16))) float f[FROWS_MAX * FD];
  const int b = blockIdx.x, tid = threadIdx.x, c = tid & 63, g = tid >> 6;
  const int P = a.P, NP = P * P, T = NP + 1;
  const int nk[3] = {NP / 4, NP, 9 * NP / 4};
  const int off[3] = {0, NP / 4, NP / 4 + NP};
  const float s1 = *a.xs1, s2 = *a.xs2;
#pragma unroll
  for (int k = 0; k < 3; ++k)
    for (int i = tid; i < nk[k] * FD; i += 256) {
      const long src = (long)b * nk[k] * FD + i;
      f[off[k] * FD + i] = a.pa[k][src] * s1 + a.pb[k][src] * s2;
    }
  __syncthreads();
  float av[FNP_MAX / 4], mx[FNP_MAX / 4];
#pragma unroll
  for (int i = 0; i < FNP_MAX / 4; ++i) {
    const int j = g + 4 * i;
    av[i] = mx[i] = 0.f;
    if (j >= NP) continue;
    float ev[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float* w = a.W[k] + (long)j * nk[k];
      float acc = 0.f;
      for (int p = 0; p < nk[k]; ++p) acc += w[p] * f[(off[k] + p) * FD + c];
      acc += a.bias[k][j];
      ev[k] = acc;
      a.e[(((long)k * a.B + b) * NP + j) * FD + c] = acc;
    }
    av[i] = (ev[0] + ev[1] + ev[2]) * (1.0f / 3.0f);
    mx[i] = fmaxf(fmaxf(ev[0], ev[1]), ev[2]);
  }
  __syncthreads();
  float* A = f;
  float* M = f + FNP_MAX * FD;
#pragma unroll
  for (int i = 0; i < FNP_MAX / 4; ++i) {
    const int j = g + 4 * i;
    if (j < NP) {
      A[j * FD + c] = av[i];
      M[j * FD + c] = mx[i];
    }
  }
  __syncthreads();
  const float p0 = a.pos[c];
  for (int j = g; j < NP; j += 4) {
    const int jy = j / P, jx = j - jy * P;
    float acc = 0.f;
    for (int ty = 0; ty < 7; ++ty) {
      const int y = jy + ty - 3;
      if (y < 0 || y >= P) continue;
      for (int tx = 0; tx < 7; ++tx) {
        const int x = jx + tx - 3;
        if (x < 0 || x >= P) continue;
        acc += a.w7[ty * 7 + tx] * A[(y * P + x) * FD + c] + a.w7[49 + ty * 7 + tx] * M[(y * P + x) * FD + c];
      }
    }
    const float s = sigmoid_exact(acc);
    a.xcnn[((long)b * NP + j) * FD + c] = s;
    a.X0[((long)b * T + 1 + j) * FD + c] = (s + a.pos[(1 + j) * FD + c]) + p0;
  }
  if (g == 0) a.X0[(long)b * T * FD + c] = a.cls[c] + p0;
}

constexpr int FK_PITCH = FD + 1;
constexpr int FUSE_BWD_LDS = FNP_MAX * FD + (9 * FNP_MAX / 4) * FK_PITCH;   // de + the scale's fused map: 13,456 floats

__global__ __launch_bounds__(256) void fuse_bwd(FuseArgs a) {
  __shared__ __attribute__((aligned(16))) float sh[FUSE_BWD_LDS];
  __shared__ float red[98 * 4];
  __shared__ float red2[8];
  const int b = blockIdx.x, tid = threadIdx.x, c = tid & 63, g = tid >> 6, lane = tid & 63;
  const int P = a.P, NP = P * P, T = NP + 1;
  const int nk[3] = {NP / 4, NP, 9 * NP / 4};
  const long width = (long)NP * (nk[0] + nk[1] + nk[2]) + 3 * NP + 100;
  float* pr = a.part + (long)b * width;
  float* gz = sh;
  float* A = sh + FNP_MAX * FD;
  float* M = sh + 2 * FNP_MAX * FD;
  // phase 1: d(pre-sigmoid) of the 7x7 conv's output and the conv's two input maps, recomputed from the saved e
  int am[FNP_MAX / 4];
#pragma unroll
  for (int i = 0; i < FNP_MAX / 4; ++i) {
    const int j = g + 4 * i;
    am[i] = 0;
    if (j >= NP) continue;
    const float s = a.xcnn[((long)b * NP + j) * FD + c];
    const float d = a.dX0[((long)b * T + 1 + j) * FD + c] + a.dxcnn[((long)b * NP + j) * FD + c];
    gz[j * FD + c] = d * s * (1.0f - s);
    float ev[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) ev[k] = a.e[(((long)k * a.B + b) * NP + j) * FD + c];
    A[j * FD + c] = (ev[0] + ev[1] + ev[2]) * (1.0f / 3.0f);
    int arg = 0;
    float m = ev[0];
    if (ev[1] > m) { m = ev[1]; arg = 1; }
    if (ev[2] > m) { m = ev[2]; arg = 2; }
    M[j * FD + c] = m;
    am[i] = arg;
  }
  __syncthreads();
  // the 7x7 kernel's gradient: 98 sums over (j, c); thread partials over its j, lanes by shuffle, the 4 waves in order
  for (int t = 0; t < 98; ++t) {
    const int ch = t / 49, r = t - ch * 49, ty = r / 7, tx = r - ty * 7;
    const float* in = ch ? M : A;
    float acc = 0.f;
    for (int j = g; j < NP; j += 4) {
      const int jy = j / P, jx = j - jy * P;
      const int y = jy + ty - 3, x = jx + tx - 3;
      if (y >= 0 && y < P && x >= 0 && x < P) acc += gz[j * FD + c] * in[(y * P + x) * FD + c];
    }
    acc = wave_sum(acc);
    if (lane == 0) red[t * 4 + g] = acc;
  }
  // phase 2: the conv's input gradients at this thread's (j, c)
  float da[FNP_MAX / 4], dm[FNP_MAX / 4];
#pragma unroll
  for (int i = 0; i < FNP_MAX / 4; ++i) {
    const int j = g + 4 * i;
    da[i] = dm[i] = 0.f;
    if (j >= NP) continue;
    const int jy = j / P, jx = j - jy * P;
    float s0 = 0.f, s1 = 0.f;
    for (int ty = 0; ty < 7; ++ty) {
      const int y = jy - ty + 3;
      if (y < 0 || y >= P) continue;
      for (int tx = 0; tx < 7; ++tx) {
        const int x = jx - tx + 3;
        if (x < 0 || x >= P) continue;
        const float v = gz[(y * P + x) * FD + c];
        s0 += a.w7[ty * 7 + tx] * v;
        s1 += a.w7[49 + ty * 7 + tx] * v;
      }
    }
    da[i] = s0 * (1.0f / 3.0f);
    dm[i] = s1;
  }
  __syncthreads();
  if (tid < 98) pr[(long)NP * (nk[0] + nk[1] + nk[2]) + 3 * NP + tid] =
      ((red[tid * 4] + red[tid * 4 + 1]) + red[tid * 4 + 2]) + red[tid * 4 + 3];
  // phase 3: per scale, the spatial Linear backwards
  float* de = sh;
  float* fk = sh + FNP_MAX * FD;
  const float s1 = *a.xs1, s2 = *a.xs2;
  float sx1 = 0.f, sx2 = 0.f;
  long woff = 0;
  for (int k = 0; k < 3; ++k) {
    const int n = nk[k];
#pragma unroll
    for (int i = 0; i < FNP_MAX / 4; ++i) {
      const int j = g + 4 * i;
      if (j < NP) de[j * FD + c] = da[i] + (am[i] == k ? dm[i] : 0.f);
    }
    for (int i = tid; i < n * FD; i += 256) {
      const long src = (long)b * n * FD + i;
      fk[(i >> 6) * FK_PITCH + (i & 63)] = a.pa[k][src] * s1 + a.pb[k][src] * s2;
    }
    __syncthreads();
    for (int i = tid; i < NP * n; i += 256) {   // dW_k[j][p] = sum_c de[j][c] f_k[p][c]
      const int j = i / n, p = i - j * n;
      float acc = 0.f;
      for (int cc = 0; cc < FD; ++cc) acc += de[j * FD + cc] * fk[p * FK_PITCH + cc];
      pr[woff + i] = acc;
    }
    if (tid < NP) {   // db_k[j]
      float acc = 0.f;
      for (int cc = 0; cc < FD; ++cc) acc += de[tid * FD + cc];
      pr[woff + (long)NP * n + tid] = acc;
    }
    for (int p = g; p < n; p += 4) {   // df_k[p][c] = sum_j W_k[j][p] de[j][c]
      float acc = 0.f;
      for (int j = 0; j < NP; ++j) acc += a.W[k][(long)j * n + p] * de[j * FD + c];
      const long o = ((long)b * n + p) * FD + c;
      sx1 += acc * a.pa[k][o];
      sx2 += acc * a.pb[k][o];
      a.dpa[k][o] = acc * s1;
      a.dpb[k][o] = acc * s2;
    }
    woff += (long)NP * n + NP;
    __syncthreads();
  }
  sx1 = wave_sum(sx1);
  sx2 = wave_sum(sx2);
  if (lane == 0) {
    red2[g] = sx1;
    red2[4 + g] = sx2;
  }
  __syncthreads();
  if (tid < 2) pr[woff + 98 + tid] = ((red2[4 * tid] + red2[4 * tid + 1]) + red2[4 * tid + 2]) + red2[4 * tid + 3];
}

// ------------------------------------------------------------------ the decoder convolutions: upsample + 3x3
constexpr int TM = 128, TN = 128, TK = 32;
constexpr int PK = 129;   // LDS pitch of images transposed from k-contiguous rows
constexpr int PO = 132;   // LDS pitch of images stored from k-outer rows

typedef float f32x16 __attribute__((ext_vector_type(16)));

enum { FWD = 0, WGRAD = 1, DGRAD = 2 };

struct UpArgs {
  int nb, P, s, C, O, OH;        // input side P, output side OH = s P
  int Cw;                        // Wt row pitch per tap: C rounded up to 4
  int M, N;                      // GEMM output extents
  int NPIX;                      // wgrad: output pixels (the contraction)
  int nk, tpt, kper;             // k-tiles; fwd / dgrad: k-tiles per tap, wgrad: n-tiles per tap; k-tiles per slice
  const float* x;  long ldx;     // input rows [B P^2][ldx]
  const float* dy; long lddy;    // output-gradient rows [B OH^2][lddy]
  const float* w;                // Wt [O][9][Cw] (vc_conv3x3_pack mode 0)
  const float* bias;
  float* out; long ldo;          // fwd: y; wgrad: dw [O][C][3][3]; dgrad: dx
  float beta;
  float* part;                   // split-K slabs [nsplit][M][N]
  float* dbias;                  // wgrad
  int vx, vdy, vw;
  FastDiv fOH, fOHW, fP, fPP, fS;
};

__device__ __forceinline__ int tap_di(int tap) { return tap >= 6 ? 2 : (tap >= 3 ? 1 : 0); }

// the input row that output pixel (b, i, j) reads through tap t: the upsampled pixel (i + di - 1, j + dj - 1), zero
// padding outside [0, OH), divided by s
__device__ __forceinline__ int up_in_row(const UpArgs& a, int b, int i, int j, int tap) {
  const int di = tap_di(tap), dj = tap - 3 * di;
  const int y = i + di - 1, x = j + dj - 1;
  if (b < 0 || y < 0 || y >= a.OH || x < 0 || x >= a.OH) return -1;
  return (b * a.P + fdiv(y, a.fS)) * a.P + fdiv(x, a.fS);
}
// the output row that reads upsampled pixel (b, ui, uj) through tap t
__device__ __forceinline__ int up_out_row(const UpArgs& a, int b, int ui, int uj, int tap) {
  const int di = tap_di(tap), dj = tap - 3 * di;
  const int y = ui - di + 1, x = uj - dj + 1;
  return (b >= 0 && y >= 0 && y < a.OH && x >= 0 && x < a.OH) ? (b * a.OH + y) * a.OH + x : -1;
}

__device__ __forceinline__ void load4(const float* base, long ld, int row, int c, int cend, bool vec, float* v) {
  if (row < 0) {
    v[0] = v[1] = v[2] = v[3] = 0.f;
    return;
  }
  const float* p = base + (long)row * ld + c;
  if (vec && c + 3 < cend) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = c + e < cend ? p[e] : 0.f;
  }
}

//   fwd   : y[p][o]         = b[o] + sum_{tap,c} x[in(p,tap)][c] Wt[o][tap][c]          M = B OH^2, N = O, K = 9 C
//   wgrad : dw[o][c][tap]   = sum_p dy[p][o] x[in(p,tap)][c]                            M = O, N = 9 C, K = B OH^2
//   dgrad : dx[q][c]     (+)= sum_{rep,tap,o} dy[out(s q + rep, tap)][o] Wt[o][tap][c]  M = B P^2, N = C, K = s^2 9 O
template <int MODE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void upconv(UpArgs a) {
  constexpr int PA = MODE == WGRAD ? PO : PK;
  constexpr int PB = MODE == FWD ? PK : PO;
  __shared__ __attribute__((aligned(16))) float As[TK * PA];
  __shared__ __attribute__((aligned(16))) float Bs[TK * PB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, h = lane >> 5;
  const int m0 = blockIdx.y * TM;
  const int nt = blockIdx.x;
  const int kt0 = blockIdx.z * a.kper, kt1 = min(a.nk, kt0 + a.kper);
  const int ntap = MODE == WGRAD ? nt / a.tpt : 0;
  const int n0 = MODE == WGRAD ? (nt - ntap * a.tpt) * TN : nt * TN;
  const int Kt = MODE == FWD ? a.C : a.O;
  const int kr = tid >> 3, kc = tid & 7;
  const int ok = tid >> 5, oc = tid & 31;
  int rb_[4], ri_[4], rj_[4];
  if constexpr (MODE != WGRAD) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = m0 + kr + 32 * i;
      if (r < a.M) {
        int r1;
        if (MODE == FWD) {
          rb_[i] = fdivmod(r, a.fOHW, r1);
          ri_[i] = fdivmod(r1, a.fOH, rj_[i]);
        } else {
          rb_[i] = fdivmod(r, a.fPP, r1);
          ri_[i] = fdivmod(r1, a.fP, rj_[i]);
        }
      } else {
        rb_[i] = -1; ri_[i] = rj_[i] = 0;
      }
    }
  }

  float ra[16], rbv[16];
  auto load = [&](int kt) {
    if constexpr (MODE == WGRAD) {
      const int p0 = kt * TK;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int p = p0 + ok + 8 * i;
        load4(a.dy, a.lddy, p < a.NPIX ? p : -1, m0 + 4 * oc, a.O, a.vdy, ra + 4 * i);
        int row = -1;
        if (p < a.NPIX) {
          int r1, y, x;
          const int b = fdivmod(p, a.fOHW, r1);
          y = fdivmod(r1, a.fOH, x);
          row = up_in_row(a, b, y, x, ntap);
        }
        load4(a.x, a.ldx, row, n0 + 4 * oc, a.C, a.vx, rbv + 4 * i);
      }
    } else {
      int rep = 0, rest = kt;
      if (MODE == DGRAD) {
        rep = kt / (9 * a.tpt);
        rest = kt - rep * 9 * a.tpt;
      }
      const int tap = rest / a.tpt, c0 = (rest - tap * a.tpt) * TK;
      const int ry = rep / a.s, rx = rep - ry * a.s;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (MODE == FWD) {
          const int row = up_in_row(a, rb_[i], ri_[i], rj_[i], tap);
          load4(a.x, a.ldx, row, c0 + 4 * kc, Kt, a.vx, ra + 4 * i);
          const int o = n0 + kr + 32 * i;
          load4(a.w + (long)tap * a.Cw, 9L * a.Cw, o < a.O ? o : -1, c0 + 4 * kc, a.Cw, a.vw, rbv + 4 * i);
        } else {
          const int row = up_out_row(a, rb_[i], ri_[i] * a.s + ry, rj_[i] * a.s + rx, tap);
          load4(a.dy, a.lddy, row, c0 + 4 * kc, Kt, a.vdy, ra + 4 * i);
          const int o = c0 + ok + 8 * i;
          load4(a.w + (long)tap * a.Cw, 9L * a.Cw, o < a.O ? o : -1, n0 + 4 * oc, a.Cw, a.vw, rbv + 4 * i);
        }
      }
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if constexpr (MODE == WGRAD) {
        *reinterpret_cast<float4*>(As + (ok + 8 * i) * PA + 4 * oc) =
            make_float4(ra[4 * i], ra[4 * i + 1], ra[4 * i + 2], ra[4 * i + 3]);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) As[(4 * kc + e) * PA + kr + 32 * i] = ra[4 * i + e];
      }
      if constexpr (MODE == FWD) {
#pragma unroll
        for (int e = 0; e < 4; ++e) Bs[(4 * kc + e) * PB + kr + 32 * i] = rbv[4 * i + e];
      } else {
        *reinterpret_cast<float4*>(Bs + (ok + 8 * i) * PB + 4 * oc) =
            make_float4(rbv[4 * i], rbv[4 * i + 1], rbv[4 * i + 2], rbv[4 * i + 3]);
      }
    }
  };

  // wgrad bias gradient: the blocks of n-tile 0 also sum their staged dy^T tile over k (fixed order)
  const bool do_b = MODE == WGRAD && a.dbias && blockIdx.x == 0;
  float bacc = 0.f;
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  if (kt0 < kt1) {
    load(kt0);
    for (int kt = kt0; kt < kt1; ++kt) {
      store();
      __syncthreads();
      if (kt + 1 < kt1) load(kt + 1);
      if (do_b) {
        const int mm = tid & 127, hh = tid >> 7;
#pragma unroll
        for (int k = 0; k < TK / 2; ++k) bacc += As[(hh * (TK / 2) + k) * PA + mm];
      }
#pragma unroll
      for (int ks = 0; ks < TK / 2; ++ks) {
        const int k = 2 * ks + h;
        const float a0 = As[k * PA + wm * 64 + l31];
        const float a1 = As[k * PA + wm * 64 + 32 + l31];
        const float b0 = Bs[k * PB + wn * 64 + l31];
        const float b1 = Bs[k * PB + wn * 64 + 32 + l31];
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
      }
      __syncthreads();
    }
  }

  // C/D of 32x32: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
  const bool split = gridDim.z > 1;
  if (do_b) {
    const int mm = tid & 127, hh = tid >> 7;
    if (hh == 1) Bs[mm] = bacc;
    __syncthreads();
    const int row = m0 + mm;
    if (hh == 0 && row < a.M) {
      const float v = bacc + Bs[mm];
      if (split) a.part[((long)blockIdx.z * a.M + row) * a.N + 9 * a.C] = v;
      else a.dbias[row] = v;
    }
  }
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      asm volatile("" ::: "memory");
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm * 64 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        const int cl = n0 + wn * 64 + ni * 32 + l31;
        int col;
        bool ok_ = row < a.M;
        if (MODE == WGRAD) {
          ok_ = ok_ && cl < a.C;
          col = ntap * a.C + cl;
        } else {
          ok_ = ok_ && cl < (MODE == FWD ? a.O : a.C);
          col = cl;
        }
        if (!ok_) continue;
        const float v = acc[mi][ni][r];
        if (split) {
          a.part[((long)blockIdx.z * a.M + row) * a.N + col] = v;
        } else if (MODE == WGRAD) {
          a.out[((long)row * a.C + cl) * 9 + ntap] = v;
        } else {
          float* o = a.out + (long)row * a.ldo + col;
          if (MODE == FWD) *o = v + (a.bias ? a.bias[col] : 0.f);
          else *o = (a.beta != 0.f ? a.beta * *o : 0.f) + v;
        }
      }
    }
}

// split-K combine in slice order, then the mode's epilogue
template <int MODE>
__global__ __launch_bounds__(256) void upconv_reduce(UpArgs a, int nsplit) {
  const long slab = (long)a.M * a.N;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= slab) return;
  float s = 0.f;
#pragma unroll 8
  for (int z = 0; z < nsplit; ++z) s += a.part[z * slab + e];
  const int row = (int)(e / a.N), col = (int)(e - (long)row * a.N);
  if (MODE == WGRAD) {
    if (col == 9 * a.C) {
      a.dbias[row] = s;
      return;
    }
    const int tap = col / a.C, c = col - tap * a.C;
    a.out[((long)row * a.C + c) * 9 + tap] = s;
    return;
  }
  float* o = a.out + (long)row * a.ldo + col;
  if (MODE == FWD) *o = s + (a.bias ? a.bias[col] : 0.f);
  else *o = (a.beta != 0.f ? a.beta * *o : 0.f) + s;
}

bool vec_ok(const float* p, long ld) { return p && ((uintptr_t)p % 16 == 0) && (ld % 4 == 0); }

template <int MODE>
int launch_up(UpArgs& a, int grid_n, int grid_m, float* ws, long ws_floats, hipStream_t stream) {
  // split K so that the grid fills one round of resident blocks (256 CUs x 3 blocks); slices of >= 4 k-tiles
  const long tiles = (long)grid_n * grid_m;
  const long target = 768;
  int nsplit = 1;
  if (ws && tiles < target && a.nk >= 8) {
    nsplit = (int)std::max<long>(1, std::min<long>(target / tiles, a.nk / 4));
    while (nsplit > 1 && (long)nsplit * a.M * a.N > ws_floats) --nsplit;
  }
  a.kper = vc_cdiv(a.nk, nsplit);
  nsplit = vc_cdiv(a.nk, a.kper);
  a.part = nsplit > 1 ? ws : nullptr;
  VC_REQUIRE(grid_m < 65536 && nsplit < 65536);
  hipLaunchKernelGGL(upconv<MODE>, dim3(grid_n, grid_m, nsplit), dim3(256), 0, stream, a);
  VC_CHECK_LAUNCH();
  if (nsplit > 1) {
    hipLaunchKernelGGL(upconv_reduce<MODE>, dim3(vc_cdiv((long)a.M * a.N, 256)), dim3(256), 0, stream, a, nsplit);
    VC_CHECK_LAUNCH();
  }
  return VC_OK;
}

// ---- upconv_pipe: the same three implicit GEMMs on the LDS-DMA pipeline (conv_tap.hip's conv_pipe, mfma_tiles.h):
// 64 x 64 output tiles on 8 waves, a 2-stage ring of 32-wide k-tiles filled by buffer_load ... lds (one 16-B chunk per
// lane), one barrier per k-tile, v_mfma_f32_16x16x4_f32.  The upsample lives in the per-lane DMA offsets; rows outside
// the padded upsampled image, channels past C / O and pixels past the slice get an offset past the buffer's end (the
// DMA writes zeros).  Needs O, C, ldx, lddy multiples of 4 and 16-B aligned bases (otherwise upconv above); at
// O = 144, C = 64 its 64-wide tiles waste a quarter of the MFMAs where the 128-wide ones waste half to three quarters.
constexpr int CP_B = 64;

template <int MODE>
__global__ __launch_bounds__(512) void upconv_pipe(UpArgs a, int tn, int nsplit, unsigned total) {
  constexpr int NW = 8, BM = CP_B, BN = CP_B, WN = NW / 2, NS = 2, QN = 8 / NW;
  constexpr int WTM = BM / 2, WTN = BN / WN, MT = WTM / 16, NT = WTN / 16;
  constexpr int SA_B = BM * 128, STAGE = (BM + BN) * 128;
  constexpr bool TA = MODE == WGRAD;   // A image [k][m] (row-contiguous) for the weight gradient
  constexpr bool TB = MODE != FWD;     // B image [k][n] for the data and weight gradients
  typedef g2::Stage<false, TA, BM, false> SA;
  typedef g2::Stage<false, TB, BN, false> SB;
  __shared__ __attribute__((aligned(1024))) char smem[gp::ring_bytes<BM, BN, NS>()];
  __shared__ float bsh[NW][64];
  int zs, xn, ym, zb;
  const int tm = (a.M + BM - 1) / BM;
  gp::tile_coords(gp::xcd_linear(blockIdx.x, total), nsplit, tn, tm, 1, zs, xn, ym, zb);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int m0 = ym * BM;
  const int ntap = MODE == WGRAD ? xn / a.tpt : 0;
  const int n0 = MODE == WGRAD ? (xn - ntap * a.tpt) * BN : xn * BN;
  const int kt0 = zs * a.kper, kt1 = min(a.nk, kt0 + a.kper);
  const unsigned OOB = gp::OOB;
  const long in_rows = (long)a.nb * a.P * a.P, out_rows = (long)a.nb * a.OH * a.OH;
  const auto rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x), (short)0,
                                                    a.x ? (int)(in_rows * a.ldx * 4) : 0, 0x00020000);
  const auto rdy = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.dy), (short)0,
                                                     a.dy ? (int)(out_rows * a.lddy * 4) : 0, 0x00020000);
  const auto rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.w), (short)0,
                                                    a.w ? (int)((long)a.O * 9 * a.Cw * 4) : 0, 0x00020000);
  // K-contiguous fills (FWD A / B, DGRAD A): this lane's image row, decomposed once
  int kb_[QN], ki_[QN], kj_[QN];
  bool kok_[QN];
  if constexpr (MODE != WGRAD) {
#pragma unroll
    for (int q = 0; q < QN; ++q) {
      const int rloc = 8 * (wave + NW * q) + (lane >> 3);
      const int m = m0 + rloc;
      kok_[q] = m < a.M;
      int r1;
      if (MODE == FWD) {
        kb_[q] = fdivmod(kok_[q] ? m : 0, a.fOHW, r1);
        ki_[q] = fdivmod(r1, a.fOH, kj_[q]);
      } else {
        kb_[q] = fdivmod(kok_[q] ? m : 0, a.fPP, r1);
        ki_[q] = fdivmod(r1, a.fP, kj_[q]);
      }
    }
  }
  auto issue = [&](int t) {
    char* st = smem + (t % NS) * STAGE;
    const int kt = kt0 + t;
#pragma unroll
    for (int q = 0; q < QN; ++q) {
      const int i = wave + NW * q;   // wave-instruction: 1 KB of each image
      const int rloc = 8 * i + (lane >> 3), kk = 4 * ((lane & 7) ^ ((rloc >> 1) & 7));
      const int kr = 4 * i + (lane >> 4), sq = lane & 15;
      const int col = (((sq >> 2) ^ ((kr >> 2) & 1)) << 4) + ((sq & 3) << 2);
      unsigned va, vb;
      if constexpr (MODE == FWD) {
        const int tap = kt / a.tpt, c = (kt - tap * a.tpt) * 32 + kk;
        const int row = up_in_row(a, kb_[q], ki_[q], kj_[q], tap);
        va = (kok_[q] && row >= 0 && c < a.C) ? (unsigned)(((long)row * a.ldx + c) * 4) : OOB;
        const int o = n0 + rloc;
        vb = (o < a.O && c < a.Cw) ? (unsigned)(((long)o * 9 * a.Cw + (long)tap * a.Cw + c) * 4) : OOB;
      } else if constexpr (MODE == DGRAD) {
        const int rep = kt / (9 * a.tpt), rest = kt - rep * 9 * a.tpt;
        const int tap = rest / a.tpt, o0 = (rest - tap * a.tpt) * 32;
        const int ry = rep / a.s, rx_ = rep - ry * a.s;
        const int row = up_out_row(a, kb_[q], ki_[q] * a.s + ry, kj_[q] * a.s + rx_, tap), o = o0 + kk;
        va = (kok_[q] && row >= 0 && o < a.O) ? (unsigned)(((long)row * a.lddy + o) * 4) : OOB;
        const int ob = o0 + kr, c = n0 + col;
        vb = (ob < a.O && c < a.Cw) ? (unsigned)(((long)ob * 9 * a.Cw + (long)tap * a.Cw + c) * 4) : OOB;
      } else {
        const int p = kt * 32 + kr, o = m0 + col, c = n0 + col;
        va = (p < a.NPIX && o < a.O) ? (unsigned)(((long)p * a.lddy + o) * 4) : OOB;
        int row = -1;
        if (p < a.NPIX) {
          int r1, y, x;
          const int b = fdivmod(p, a.fOHW, r1);
          y = fdivmod(r1, a.fOH, x);
          row = up_in_row(a, b, y, x, ntap);
        }
        vb = (row >= 0 && c < a.C) ? (unsigned)(((long)row * a.ldx + c) * 4) : OOB;
      }
      if constexpr (MODE == FWD) gp::dma16(rx, st + i * 1024, va);
      else gp::dma16(rdy, st + i * 1024, va);
      if constexpr (MODE == WGRAD) gp::dma16(rx, st + SA_B + i * 1024, vb);
      else gp::dma16(rw, st + SA_B + i * 1024, vb);
    }
  };
  f32x4 acc[1][MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[0][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // weight gradient's bias column: the n-tile-0 blocks sum their staged dy tile (A, [k][m]) over k -- thread
  // (m = tid & 63, k group tid >> 6), k-tiles in order, the groups in order at the end
  const bool do_b = MODE == WGRAD && a.dbias && xn == 0;
  float bacc = 0.f;
  const int nk = kt1 > kt0 ? kt1 - kt0 : 0;
  if (nk > 0) issue(0);
  for (int t = 0; t < nk; ++t) {
    gp::vm_wait<0>();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's reads of the slot refilled below
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (t + 1 < nk) issue(t + 1);
    const char* cur = smem + (t % NS) * STAGE;
    if (do_b) {
      const int mm = tid & 63, kq = tid >> 6;
#pragma unroll
      for (int k = 0; k < 32 / NW; ++k)
        bacc += *reinterpret_cast<const float*>(cur + SA::rc_off((32 / NW) * kq + k, mm));
    }
    g2::mma_ktile<false, MT, NT, SA, SB, 1>(cur, cur + SA_B, wm * WTM, wn * WTN, lane, acc);
  }
  const bool split = nsplit > 1;
  if (do_b) {
    const int mm = tid & 63, kq = tid >> 6;
    bsh[kq][mm] = bacc;
    __syncthreads();
    const int row = m0 + mm;
    if (kq == 0 && row < a.M) {
      float v = bsh[0][mm];
#pragma unroll
      for (int w2 = 1; w2 < NW; ++w2) v += bsh[w2][mm];   // the k groups in order
      if (split) a.part[((long)zs * a.M + row) * a.N + 9 * a.C] = v;
      else a.dbias[row] = v;
    }
  }
  // C/D map of the 16x16 MFMAs: col = lane & 15, row = (lane >> 4) * 4 + r
#pragma unroll
  for (int mi = 0; mi < MT; ++mi)
#pragma unroll
    for (int ni = 0; ni < NT; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + wm * WTM + mi * 16 + (lane >> 4) * 4 + r;
        const int nl = n0 + wn * WTN + ni * 16 + (lane & 15);
        const int nmax = MODE == FWD ? a.O : a.C;
        if (m >= a.M || nl >= nmax) continue;
        const float v = acc[0][mi][ni][r];
        const int col = MODE == WGRAD ? ntap * a.C + nl : nl;
        if (split) {
          a.part[((long)zs * a.M + m) * a.N + col] = v;
        } else if (MODE == WGRAD) {
          a.out[((long)m * a.C + nl) * 9 + ntap] = v;
        } else {
          float* o = a.out + (long)m * a.ldo + col;
          if (MODE == FWD) *o = v + (a.bias ? a.bias[col] : 0.f);
          else *o = (a.beta != 0.f ? a.beta * *o : 0.f) + v;
        }
      }
}

// the pipelined kernel's launch: split K (slices of >= 4 k-tiles) only for small grids, conv_tap.hip's plan
template <int MODE>
int launch_up_pipe(UpArgs& a, int grid_n, float* ws, long ws_floats, hipStream_t stream) {
  const int tm = vc_cdiv(a.M, CP_B);
  const long tiles = (long)grid_n * tm;
  static const long below_default[3] = {512, 1024, 512};
  const long below = below_default[MODE];
  int nsplit = 1;
  if (ws && tiles < below)
    nsplit = (int)std::max<long>(1, std::min<long>(std::min<long>((4 * below + tiles - 1) / tiles, a.nk / 4), 64));
  while (nsplit > 1 && (long)nsplit * a.M * a.N > ws_floats) --nsplit;
  a.kper = vc_cdiv(a.nk, nsplit);
  nsplit = vc_cdiv(a.nk, a.kper);
  a.part = nsplit > 1 ? ws : nullptr;
  const long total = tiles * nsplit;
  VC_REQUIRE(total < (1L << 31));
  hipLaunchKernelGGL(upconv_pipe<MODE>, dim3((unsigned)total), dim3(512), 0, stream, a, grid_n, nsplit, (unsigned)total);
  VC_CHECK_LAUNCH();
  if (nsplit > 1) {
    hipLaunchKernelGGL(upconv_reduce<MODE>, dim3(vc_cdiv((long)a.M * a.N, 256)), dim3(256), 0, stream, a, nsplit);
    VC_CHECK_LAUNCH();
  }
  return VC_OK;
}

// whole 16-B chunks everywhere and operands under 2 GB (32-bit buffer offsets)
bool up_pipe_ok(const UpArgs& a, const void* p0, long ld0, const void* p1, long ld1) {
  const long in_b = (long)a.nb * a.P * a.P * 4, out_b = (long)a.nb * a.OH * a.OH * 4;
  return a.O % 4 == 0 && a.C % 4 == 0 && ld0 % 4 == 0 && ld1 % 4 == 0 && ((uintptr_t)p0 % 16) == 0 &&
         ((uintptr_t)p1 % 16) == 0 && in_b * std::max(ld0, ld1) < (1L << 31) && out_b * std::max(ld0, ld1) < (1L << 31) &&
         (long)a.O * 9 * a.Cw * 4 < (1L << 31);
}

int up_geo(UpArgs& a, int B, int P, int s, int C, int O) {
  VC_REQUIRE(B > 0 && P >= 1 && s >= 1 && s <= 3 && C > 0 && O > 0);
  a = UpArgs{};
  a.nb = B; a.P = P; a.s = s; a.C = C; a.O = O; a.OH = s * P;
  a.Cw = (C + 3) & ~3;
  a.fOH = make_fastdiv(a.OH); a.fOHW = make_fastdiv(a.OH * a.OH);
  a.fP = make_fastdiv(P); a.fPP = make_fastdiv(P * P); a.fS = make_fastdiv(s);
  return VC_OK;
}

// ------------------------------------------------------------------ sigmoid + MSE
constexpr int SM_PER_BLOCK = 256 * 8;

// element indices are 32-bit (rows * ld < 2^31 is checked on the host) and split by a launch-time fast division
__global__ __launch_bounds__(256) void sigmse_fwd(int n, FastDiv fC, float* __restrict__ y, long ldy,
                                                  const float* __restrict__ t, long ldt, double scale, int accumulate,
                                                  double* __restrict__ ws, unsigned int* cnt, float* __restrict__ loss) {
  __shared__ double sh[256];
  const int e0 = blockIdx.x * SM_PER_BLOCK;
  double acc = 0.0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int e = e0 + i * 256 + threadIdx.x;
    if (e < n) {
      int c;
      const long r = fdivmod(e, fC, c);
      const float s = sigmoid_exact(y[r * ldy + c]);
      y[r * ldy + c] = s;
      const float d = s - t[r * ldt + c];
      acc += (double)d * (double)d;
    }
  }
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) ws[blockIdx.x] = sh[0];
  if (block_last_arriver(cnt, gridDim.x)) {
    if (threadIdx.x == 0) {
      double s = 0.0;
      for (unsigned i = 0; i < gridDim.x; ++i) s += ws[i];   // the blocks in order
      *loss = (accumulate ? *loss : 0.f) + (float)(s * scale);
    }
  }
}

__global__ __launch_bounds__(256) void sigmse_bwd(int n, FastDiv fC, const float* __restrict__ sg, long lds,
                                                  const float* __restrict__ t, long ldt, float scale2,
                                                  const float* __restrict__ dloss, float* __restrict__ d, long ldd) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  int c;
  const long r = fdivmod(e, fC, c);
  const float s = sg[r * lds + c];
  d[r * ldd + c] = (*dloss * scale2) * (s - t[r * ldt + c]) * s * (1.0f - s);
}

// ------------------------------------------------------------------ classifier tail
__global__ __launch_bounds__(64) void tail_fwd(int n, int HW, const float* __restrict__ lg1, const float* __restrict__ z,
                                               long ldz, const float* __restrict__ W2, const float* __restrict__ b2,
                                               const float* __restrict__ c1, const float* __restrict__ c2,
                                               float* __restrict__ p2, float* __restrict__ avg, float* __restrict__ out) {
  __shared__ float av[32];
  __shared__ float l2[256];
  __shared__ float st[2];
  const int b = blockIdx.x, t = threadIdx.x;
  if (t < 32) {
    float acc = 0.f;
    for (int r = 0; r < HW; ++r) acc += z[((long)b * HW + r) * ldz + t];
    acc *= 1.0f / (float)HW;
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
  if (t == 0) {   // max and sum of the softmax, serially in class order
    float m = -INFINITY;
    for (int c = 0; c < n; ++c) m = fmaxf(m, l2[c]);
    float sum = 0.f;
    for (int c = 0; c < n; ++c) sum += expf(l2[c] - m);
    st[0] = m;
    st[1] = 1.0f / sum;
  }
  __syncthreads();
  const float a1 = *c1, a2 = *c2;
  for (int c = t; c < n; c += 64) {
    const float w = expf(l2[c] - st[0]) * st[1];
    p2[(long)b * n + c] = w;
    out[(long)b * n + c] = lg1[(long)b * n + c] * a1 + w * a2;
  }
}

__global__ __launch_bounds__(64) void tail_bwd(int n, int HW, const float* __restrict__ dout, const float* __restrict__ lg1,
                                               const float* __restrict__ p2, const float* __restrict__ avg,
                                               const float* __restrict__ W2, const float* __restrict__ c1,
                                               const float* __restrict__ c2, float* __restrict__ dlg1,
                                               float* __restrict__ dz, long lddz, float* __restrict__ part) {
  __shared__ float d2[256];
  __shared__ float st[2];
  const int b = blockIdx.x, t = threadIdx.x;
  const float* go = dout + (long)b * n;
  const float* u = lg1 + (long)b * n;
  const float* w = p2 + (long)b * n;
  float* pr = part + (long)b * (n * 33 + 2);
  if (t < 2) {
    const float* src = t == 0 ? u : w;
    float acc = 0.f;
    for (int c = 0; c < n; ++c) acc += go[c] * src[c];
    st[t] = acc;
    pr[n * 33 + t] = acc;   // dc1, dc2
  }
  __syncthreads();
  const float a1 = *c1, a2 = *c2;
  for (int c = t; c < n; c += 64) {
    dlg1[(long)b * n + c] = a1 * go[c];
    const float d = a2 * w[c] * (go[c] - st[1]);
    d2[c] = d;
    pr[n * 32 + c] = d;
  }
  __syncthreads();
  for (int i = t; i < n * 32; i += 64) pr[i] = d2[i / 32] * avg[b * 32 + i % 32];
  if (t < 32) {
    float acc = 0.f;
    for (int c = 0; c < n; ++c) acc += d2[c] * W2[c * 32 + t];
    acc *= 1.0f / (float)HW;
    for (int r = 0; r < HW; ++r) dz[((long)b * HW + r) * lddz + t] = acc;
  }
}

bool fuse_ok(int B, int P) { return B > 0 && P >= 2 && P <= FP_MAX && P % 2 == 0; }

}  // namespace

VC_API int vc_glt_crops(int B, int C, int P, const float* x, float* r1, float* r2, float* r3, int ld,
                        hipStream_t stream) {
  VC_REQUIRE(B > 0 && C > 0 && P >= 2 && P % 2 == 0 && ld >= C && x && r1 && r2 && r3);
  const long total = (long)B * 14 * P * P * ld;
  VC_REQUIRE_I32(total);
  VC_REQUIRE_I32((long)B * C * 9 * P * P);
  hipLaunchKernelGGL(crops_kernel, dim3(vc_cdiv(total, 256)), dim3(256), 0, stream, B, C, P, ld, total, x, r1, r2, r3);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

VC_API int vc_glt_fuse_part_floats(int P) {
  if (P < 2 || P > FP_MAX || P % 2) return -1;
  const int NP = P * P;
  return NP * (NP / 4 + NP + 9 * NP / 4) + 3 * NP + 100;
}

VC_API int vc_glt_fuse_fwd(int B, int P, const float* pa1, const float* pb1, const float* pa2, const float* pb2,
                           const float* pa3, const float* pb3, const float* xs1, const float* xs2, const float* W1,
                           const float* b1, const float* W2, const float* b2, const float* W3, const float* b3,
                           const float* w7, const float* pos, const float* cls, float* xcnn, float* X0, float* e,
                           hipStream_t stream) {
  VC_REQUIRE(fuse_ok(B, P));
  VC_REQUIRE(pa1 && pb1 && pa2 && pb2 && pa3 && pb3 && xs1 && xs2 && W1 && b1 && W2 && b2 && W3 && b3 && w7 && pos &&
             cls && xcnn && X0 && e);
  FuseArgs a{};
  a.B = B; a.P = P;
  a.pa[0] = pa1; a.pa[1] = pa2; a.pa[2] = pa3;
  a.pb[0] = pb1; a.pb[1] = pb2; a.pb[2] = pb3;
  a.W[0] = W1; a.W[1] = W2; a.W[2] = W3;
  a.bias[0] = b1; a.bias[1] = b2; a.bias[2] = b3;
  a.xs1 = xs1; a.xs2 = xs2; a.w7 = w7; a.pos = pos; a.cls = cls;
  a.xcnn = xcnn; a.X0 = X0; a.e = e;
  hipLaunchKernelGGL(fuse_fwd, dim3(B), dim3(256), 0, stream, a);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

VC_API int vc_glt_fuse_bwd(int B, int P, const float* pa1, const float* pb1, const float* pa2, const float* pb2,
                           const float* pa3, const float* pb3, const float* xs1, const float* xs2, const float* W1,
                           const float* W2, const float* W3, const float* w7, const float* xcnn, const float* e,
                           const float* dX0, const float* dxcnn, float* dpa1, float* dpb1, float* dpa2, float* dpb2,
                           float* dpa3, float* dpb3, float* part, hipStream_t stream) {
  VC_REQUIRE(fuse_ok(B, P));
  VC_REQUIRE(pa1 && pb1 && pa2 && pb2 && pa3 && pb3 && xs1 && xs2 && W1 && W2 && W3 && w7 && xcnn && e && dX0 && dxcnn &&
             dpa1 && dpb1 && dpa2 && dpb2 && dpa3 && dpb3 && part);
  FuseArgs a{};
  a.B = B; a.P = P;
  a.pa[0] = pa1; a.pa[1] = pa2; a.pa[2] = pa3;
  a.pb[0] = pb1; a.pb[1] = pb2; a.pb[2] = pb3;
  a.W[0] = W1; a.W[1] = W2; a.W[2] = W3;
  a.xs1 = xs1; a.xs2 = xs2; a.w7 = w7;
  a.xcnn = const_cast<float*>(xcnn); a.e = const_cast<float*>(e);
  a.dX0 = dX0; a.dxcnn = dxcnn;
  a.dpa[0] = dpa1; a.dpa[1] = dpa2; a.dpa[2] = dpa3;
  a.dpb[0] = dpb1; a.dpb[1] = dpb2; a.dpb[2] = dpb3;
  a.part = part;
  hipLaunchKernelGGL(fuse_bwd, dim3(B), dim3(256), 0, stream, a);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

VC_API int vc_glt_upconv_fwd(int B, int P, int s, int C, int O, const float* x, long ldx, const float* wt,
                             const float* bias, float* y, long ldy, float* ws, long ws_floats, hipStream_t stream) {
  UpArgs a;
  if (up_geo(a, B, P, s, C, O)) return VC_EINVAL;
  VC_REQUIRE(x && wt && y && ldx >= C && ldy >= O);
  a.M = B * a.OH * a.OH;
  a.N = O;
  VC_REQUIRE_I32((long)B * P * P * ldx);
  VC_REQUIRE_I32((long)B * a.OH * a.OH * ldy);
  a.tpt = vc_cdiv(C, TK);
  a.nk = 9 * a.tpt;
  a.x = x; a.ldx = ldx; a.w = wt; a.bias = bias; a.out = y; a.ldo = ldy;
  a.vx = vec_ok(x, ldx); a.vw = vec_ok(wt, a.Cw);
  if (up_pipe_ok(a, x, ldx, wt, 4)) return launch_up_pipe<FWD>(a, vc_cdiv(O, CP_B), ws, ws_floats, stream);
  return launch_up<FWD>(a, vc_cdiv(O, TN), vc_cdiv(a.M, TM), ws, ws_floats, stream);
}

VC_API int vc_glt_upconv_wgrad(int B, int P, int s, int C, int O, const float* x, long ldx, const float* dy, long lddy,
                               float* dw, float* db, float* ws, long ws_floats, hipStream_t stream) {
  UpArgs a;
  if (up_geo(a, B, P, s, C, O)) return VC_EINVAL;
  VC_REQUIRE(x && dy && dw && db && ldx >= C && lddy >= O);
  a.M = O;
  a.N = 9 * C + 1;   // the bias-gradient column of the split slabs
  a.NPIX = B * a.OH * a.OH;
  VC_REQUIRE_I32((long)B * P * P * ldx);
  VC_REQUIRE_I32((long)a.NPIX * lddy);
  a.tpt = vc_cdiv(C, TN);
  a.nk = vc_cdiv(a.NPIX, TK);
  a.x = x; a.ldx = ldx; a.dy = dy; a.lddy = lddy; a.out = dw; a.ldo = 9L * C;
  a.dbias = db;
  a.vx = vec_ok(x, ldx); a.vdy = vec_ok(dy, lddy);
  if (up_pipe_ok(a, x, ldx, dy, lddy)) {
    a.tpt = vc_cdiv(C, CP_B);   // n-tiles per tap
    return launch_up_pipe<WGRAD>(a, 9 * a.tpt, ws, ws_floats, stream);
  }
  return launch_up<WGRAD>(a, 9 * a.tpt, vc_cdiv(O, TM), ws, ws_floats, stream);
}

VC_API int vc_glt_upconv_dgrad(int B, int P, int s, int C, int O, const float* dy, long lddy, const float* wt,
                               float beta, float* dx, long lddx, float* ws, long ws_floats, hipStream_t stream) {
  UpArgs a;
  if (up_geo(a, B, P, s, C, O)) return VC_EINVAL;
  VC_REQUIRE(dy && wt && dx && lddy >= O && lddx >= C);
  a.M = B * P * P;
  a.N = C;
  VC_REQUIRE_I32((long)a.M * lddx);
  VC_REQUIRE_I32((long)B * a.OH * a.OH * lddy);
  a.tpt = vc_cdiv(O, TK);
  a.nk = s * s * 9 * a.tpt;
  a.dy = dy; a.lddy = lddy; a.w = wt; a.out = dx; a.ldo = lddx; a.beta = beta;
  a.vdy = vec_ok(dy, lddy); a.vw = vec_ok(wt, a.Cw);
  if (up_pipe_ok(a, dy, lddy, wt, 4)) return launch_up_pipe<DGRAD>(a, vc_cdiv(C, CP_B), ws, ws_floats, stream);
  return launch_up<DGRAD>(a, vc_cdiv(C, TN), vc_cdiv(a.M, TM), ws, ws_floats, stream);
}

VC_API int vc_glt_sigmse_ws_floats(long rows, int C) {
  if (rows <= 0 || C <= 0) return -1;
  return 2 * vc_cdiv(rows * C, SM_PER_BLOCK);
}

VC_API int vc_glt_sigmse_fwd(long rows, int C, float* y, long ldy, const float* t, long ldt, float weight,
                             int accumulate, float* loss, float* ws, long ws_floats, unsigned int* counter,
                             hipStream_t stream) {
  VC_REQUIRE(rows > 0 && C > 0 && y && t && loss && ws && counter && ldy >= C && ldt >= C);
  const long n = rows * C;
  VC_REQUIRE_I32(rows * std::max(ldy, ldt) + SM_PER_BLOCK);   // 32-bit element indices, a block's overhang included
  const int blocks = vc_cdiv(n, SM_PER_BLOCK);
  VC_REQUIRE(ws_floats >= 2L * blocks && (uintptr_t)ws % 8 == 0);
  hipLaunchKernelGGL(sigmse_fwd, dim3(blocks), dim3(256), 0, stream, (int)n, make_fastdiv(C), y, ldy, t, ldt,
                     (double)weight / (double)n,
                     accumulate, reinterpret_cast<double*>(ws), counter, loss);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

VC_API int vc_glt_sigmse_bwd(long rows, int C, const float* sg, long lds, const float* t, long ldt, float weight,
                             const float* dloss, float* d, long ldd, hipStream_t stream) {
  VC_REQUIRE(rows > 0 && C > 0 && sg && t && dloss && d && lds >= C && ldt >= C && ldd >= C);
  const long n = rows * C;
  VC_REQUIRE_I32(rows * std::max(std::max(lds, ldt), ldd));
  hipLaunchKernelGGL(sigmse_bwd, dim3(vc_cdiv(n, 256)), dim3(256), 0, stream, (int)n, make_fastdiv(C), sg, lds, t, ldt,
                     (float)(2.0 * (double)weight / (double)n), dloss, d, ldd);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

VC_API int vc_glt_tail_fwd(int B, int ncls, int HW, const float* lg1, const float* z, long ldz, const float* W2,
                           const float* b2, const float* c1, const float* c2, float* p2, float* avg, float* out,
                           hipStream_t stream) {
  VC_REQUIRE(B > 0 && ncls >= 1 && ncls <= 256 && HW >= 1 && ldz >= 32);
  VC_REQUIRE(lg1 && z && W2 && b2 && c1 && c2 && p2 && avg && out);
  hipLaunchKernelGGL(tail_fwd, dim3(B), dim3(64), 0, stream, ncls, HW, lg1, z, ldz, W2, b2, c1, c2, p2, avg, out);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

VC_API int vc_glt_tail_bwd(int B, int ncls, int HW, const float* dout, const float* lg1, const float* p2,
                           const float* avg, const float* W2, const float* c1, const float* c2, float* dlg1, float* dz,
                           long lddz, float* part, hipStream_t stream) {
  VC_REQUIRE(B > 0 && ncls >= 1 && ncls <= 256 && HW >= 1 && lddz >= 32);
  VC_REQUIRE(dout && lg1 && p2 && avg && W2 && c1 && c2 && dlg1 && dz && part);
  hipLaunchKernelGGL(tail_bwd, dim3(B), dim3(64), 0, stream, ncls, HW, dout, lg1, p2, avg, W2, c1, c2, dlg1, dz, lddz,
                     part);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

// MFT comparison model (model/compare_method/MFT.py): the ops no other model has.
//   vc_mft_conv3d_fwd / _wgrad     conv5's Conv3d(1, 8, (9,3,3), padding (0,1,1)), VALU direct conv over LDS tiles
//   vc_mft_hetconv_pack / _unpack  conv6's gwc + pwc <-> one dense tap-major 3x3 weight (vc_conv3x3_tap_*)
//   vc_mft_tokpool_fwd / _bwd      the tokenisers: softmax-over-pixels pooling, L tokens per sample
//   vc_mft_xattn_fwd / _bwd        MCrossAttention's single-query core with the per-slice projections fused
//   vc_mft_bcast_add_fwd / _bwd    the Block's broadcast residual
//   vc_adam                        torch.optim.Adam with coupled L2 weight decay over the flat buffer
// All fp32 with fp32 accumulation; every cross-block sum goes through per-block partials reduced in a fixed order
// (launch_sum_rows), so results are run-to-run identical.
#include "common.h"

#define MFT_F 64           // feature width (FM * 4)
#define MFT_HEADS 8
#define MFT_TMAX 16
#define MFT_HW_MAX 1024
#define MFT_LMAX 4

// ---------------------------------------------------------------- conv5: Conv3d(1, 8, (9,3,3), padding (0,1,1))
// One block per (sample, chunk of DT output depths): the DT + 8 input planes, zero-padded to (P+2)^2, sit in LDS with
// the 81 x 8 weights ([tap][c]: two 16-B broadcast reads per tap).  The wgrad also stages the block's dy tile.
#define C3_W 648                 // 8 * 81 weights
#define C3_PART 656              // + 8 bias sums: one block's wgrad partial
#define C3_LDS_FLOATS 15360      // 60 KB of dynamic LDS

// the depth chunk: the largest DT <= 8 whose forward and wgrad tiles fit the LDS budget (0: P unsupported)
static inline int c3_dt(int D, int P) {
  for (int dt = std::min(8, D); dt >= 1; --dt)
    if ((long)(dt + 8) * (P + 2) * (P + 2) + (long)dt * P * P * 8 + C3_W <= C3_LDS_FLOATS) return dt;
  return 0;
}

__device__ __forceinline__ void c3_load_x(float* xt, const float* __restrict__ x, int b, int NC, int P, int d0,
                                          int nplanes) {
  const int PP = P + 2, plane = PP * PP;
  for (int i = threadIdx.x; i < nplanes * plane; i += blockDim.x) {
    const int pl = i / plane, r = i - pl * plane;
    const int hh = r / PP - 1, ww = r % PP - 1;
    float v = 0.f;
    if (hh >= 0 && hh < P && ww >= 0 && ww < P) v = x[((long)b * NC + d0 + pl) * P * P + hh * P + ww];
    xt[i] = v;
  }
}

static __global__ __launch_bounds__(256) void mft_conv3d_fwd(int NC, int P, int D, int DT, const float* __restrict__ x,
                                                             const float* __restrict__ w,
                                                             const float* __restrict__ bias, float* __restrict__ y,
                                                             long ldy) {
  extern __shared__ float sm[];
  float* wsm = sm;          // [81][8]
  float* xt = sm + C3_W;    // [dt + 8][P + 2][P + 2]
  const int b = blockIdx.y, d0 = blockIdx.x * DT;
  const int dt = min(DT, D - d0);
  const int PP = P + 2, plane = PP * PP;
  for (int i = threadIdx.x; i < C3_W; i += blockDim.x) {
    const int c = i / 81, tap = i - c * 81;
    wsm[tap * 8 + c] = w[i];
  }
  c3_load_x(xt, x, b, NC, P, d0, dt + 8);
  __syncthreads();
  float bv[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) bv[c] = bias[c];
  for (int o = threadIdx.x; o < dt * P * P; o += blockDim.x) {
    const int pix = o / dt, dl = o - pix * dt;   // depth fastest: a pixel's 8 dt outputs are contiguous
    const int h = pix / P, wc = pix - h * P;
    float acc[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] = bv[c];
    for (int kd = 0; kd < 9; ++kd) {
      const float* xp = xt + (dl + kd) * plane + h * PP + wc;
      const float* wp = wsm + kd * 72;
#pragma unroll
      for (int kh = 0; kh < 3; ++kh) {
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          const float xv = xp[kh * PP + kw];
          const float4 w0 = *reinterpret_cast<const float4*>(wp + (kh * 3 + kw) * 8);
          const float4 w1 = *reinterpret_cast<const float4*>(wp + (kh * 3 + kw) * 8 + 4);
          acc[0] += xv * w0.x;
          acc[1] += xv * w0.y;
          acc[2] += xv * w0.z;
          acc[3] += xv * w0.w;
          acc[4] += xv * w1.x;
          acc[5] += xv * w1.y;
          acc[6] += xv * w1.z;
          acc[7] += xv * w1.w;
        }
      }
    }
    float* yp = y + ((long)b * P * P + pix) * ldy + (d0 + dl) * 8;
    *reinterpret_cast<float4*>(yp) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    *reinterpret_cast<float4*>(yp + 4) = make_float4(acc[4], acc[5], acc[6], acc[7]);
  }
}

// part[block][c * 81 + tap] (648) then [648 + c] (the bias sums) of this block's (sample, depth chunk)
static __global__ __launch_bounds__(256) void mft_conv3d_wgrad(int NC, int P, int D, int DT,
                                                               const float* __restrict__ x,
                                                               const float* __restrict__ dy, long lddy,
                                                               float* __restrict__ part) {
  extern __shared__ float sm[];
  const int b = blockIdx.y, d0 = blockIdx.x * DT;
  const int dt = min(DT, D - d0);
  const int PP = P + 2, plane = PP * PP, HW = P * P;
  float* xt = sm;                         // [dt + 8][P + 2][P + 2]
  float* dyt = sm + (DT + 8) * plane;     // [dt][P][P][8]
  c3_load_x(xt, x, b, NC, P, d0, dt + 8);
  for (int i = threadIdx.x; i < dt * HW * 8; i += blockDim.x) {
    const int c = i & 7, r = i >> 3;
    const int pix = r / dt, dl = r - pix * dt;
    dyt[(dl * HW + pix) * 8 + c] = dy[((long)b * HW + pix) * lddy + (d0 + dl) * 8 + c];
  }
  __syncthreads();
  float* out = part + ((long)blockIdx.y * gridDim.x + blockIdx.x) * C3_PART;
  for (int o = threadIdx.x; o < C3_PART; o += blockDim.x) {
    float acc = 0.f;
    if (o < C3_W) {
      const int c = o & 7, tap = o >> 3;   // c fastest: the x reads of 8 neighbouring lanes are one broadcast
      const int kd = tap / 9, kh = (tap / 3) % 3, kw = tap % 3;
      for (int dl = 0; dl < dt; ++dl) {
        const float* xp = xt + (dl + kd) * plane + kh * PP + kw;
        const float* dp = dyt + dl * HW * 8 + c;
        for (int h = 0; h < P; ++h)
          for (int wc = 0; wc < P; ++wc) acc += dp[(h * P + wc) * 8] * xp[h * PP + wc];
      }
      out[c * 81 + tap] = acc;
    } else {
      const int c = o - C3_W;
      for (int r = 0; r < dt * HW; ++r) acc += dyt[r * 8 + c];
      out[o] = acc;
    }
  }
}

static inline bool c3_shape_ok(int B, int NC, int P) { return B > 0 && NC >= 9 && NC <= 4096 && P >= 5 && P <= 28; }

VC_API int vc_mft_conv3d_ws_floats(int B, int NC, int P) {
  if (!c3_shape_ok(B, NC, P)) return -1;
  const int D = NC - 8, DT = c3_dt(D, P);
  if (DT < 1) return -1;
  const long n = (long)B * vc_cdiv(D, DT) * C3_PART;
  return n < (1L << 31) ? (int)n : -1;
}

VC_API int vc_mft_conv3d_fwd(int B, int NC, int P, const float* x, const float* w, const float* bias, float* y, long ldy,
                             hipStream_t stream) {
  VC_REQUIRE(c3_shape_ok(B, NC, P));
  const int D = NC - 8, DT = c3_dt(D, P);
  VC_REQUIRE(DT >= 1 && B <= 65535);
  VC_REQUIRE(ldy >= 8L * D && ldy % 4 == 0 && ((uintptr_t)y & 15) == 0);
  VC_REQUIRE_I32((long)B * P * P * ldy);
  VC_REQUIRE(x && w && bias && y);
  const size_t lds = sizeof(float) * (C3_W + (size_t)(DT + 8) * (P + 2) * (P + 2));
  hipLaunchKernelGGL(mft_conv3d_fwd, dim3(vc_cdiv(D, DT), B), dim3(256), lds, stream, NC, P, D, DT, x, w, bias, y, ldy);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

VC_API int vc_mft_conv3d_wgrad(int B, int NC, int P, const float* x, const float* dy, long lddy, float* dw, float* db,
                               float* ws, long ws_floats, hipStream_t stream) {
  VC_REQUIRE(c3_shape_ok(B, NC, P));
  const int D = NC - 8, DT = c3_dt(D, P);
  VC_REQUIRE(DT >= 1 && B <= 65535);
  VC_REQUIRE(lddy >= 8L * D);
  VC_REQUIRE_I32((long)B * P * P * lddy);
  const int nblk = vc_cdiv(D, DT);
  VC_REQUIRE(ws && (long)B * nblk * C3_PART <= ws_floats);
  VC_REQUIRE(x && dy && dw && db);
  const size_t lds = sizeof(float) * ((size_t)(DT + 8) * (P + 2) * (P + 2) + (size_t)DT * P * P * 8);
  hipLaunchKernelGGL(mft_conv3d_wgrad, dim3(nblk, B), dim3(256), lds, stream, NC, P, D, DT, x, dy, lddy, ws);
  VC_CHECK_LAUNCH();
  int rc = launch_sum_rows(B * nblk, C3_W, ws, C3_PART, 0, dw, 0.f, stream);
  if (rc) return rc;
  return launch_sum_rows(B * nblk, 8, ws, C3_PART, C3_W, db, 0.f, stream);
}

// ---------------------------------------------------------------- conv6: HetConv pack / unpack
// column k = d * 8 + c of the conv5 rows is torch channel ch = c * D + d (D = C / 8)
__device__ __forceinline__ int het_col(int ch, int D) {
  const int c = ch / D, d = ch - c * D;
  return d * 8 + c;
}

static __global__ void mft_hetconv_pack(int O, int C, int g, const float* __restrict__ gw, const float* __restrict__ pw,
                                        const float* __restrict__ gb, const float* __restrict__ pb,
                                        float* __restrict__ wt, float* __restrict__ bias) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int n = O * 9 * C;
  if (i < O) bias[i] = gb[i] + pb[i];
  if (i >= n) return;
  const int ch = i % C, tap = (i / C) % 9, o = i / (9 * C);
  const int cpg = C / g, opg = O / g;
  float v = 0.f;
  if (ch / cpg == o / opg) v = gw[((long)o * cpg + ch % cpg) * 9 + tap];
  if (tap == 4) v += pw[(long)o * C + ch];
  wt[((long)o * 9 + tap) * C + het_col(ch, C / 8)] = v;
}

static __global__ void mft_hetconv_unpack(int O, int C, int g, const float* __restrict__ dwt, float* __restrict__ dgw,
                                          float* __restrict__ dpw) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int cpg = C / g, opg = O / g;
  const int ng = O * cpg * 9;
  if (i < ng) {
    const int tap = i % 9, cl = (i / 9) % cpg, o = i / (9 * cpg);
    const int ch = (o / opg) * cpg + cl;
    dgw[i] = dwt[((long)o * 9 + tap) * C + het_col(ch, C / 8)];
  } else if (i < ng + O * C) {
    const int j = i - ng;
    const int ch = j % C, o = j / C;
    dpw[j] = dwt[((long)o * 9 + 4) * C + het_col(ch, C / 8)];
  }
}

static inline bool het_ok(int O, int C, int g) {
  return O > 0 && C > 0 && g > 0 && C % 8 == 0 && C % g == 0 && O % g == 0 && (long)O * 9 * C < (1L << 31);
}

VC_API int vc_mft_hetconv_pack(int O, int C, int g, const float* gwc_w, const float* pwc_w, const float* gwc_b,
                               const float* pwc_b, float* wt, float* bias, hipStream_t stream) {
  VC_REQUIRE(het_ok(O, C, g));
  VC_REQUIRE(gwc_w && pwc_w && gwc_b && pwc_b && wt && bias);
  hipLaunchKernelGGL(mft_hetconv_pack, dim3(vc_cdiv((long)O * 9 * C, 256)), dim3(256), 0, stream, O, C, g, gwc_w, pwc_w,
                     gwc_b, pwc_b, wt, bias);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

VC_API int vc_mft_hetconv_unpack(int O, int C, int g, const float* dwt, float* dgwc_w, float* dpwc_w,
                                 hipStream_t stream) {
  VC_REQUIRE(het_ok(O, C, g));
  VC_REQUIRE(dwt && dgwc_w && dpwc_w);
  const long n = (long)O * (C / g) * 9 + (long)O * C;
  hipLaunchKernelGGL(mft_hetconv_unpack, dim3(vc_cdiv(n, 256)), dim3(256), 0, stream, O, C, g, dwt, dgwc_w, dpwc_w);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

// ---------------------------------------------------------------- tokenisers
// One block (256 threads = 4 waves) per sample; wave l owns token l's softmax.
__device__ __forceinline__ void tok_dots(const float* __restrict__ xr, const float (*wl)[MFT_F], int L, float* out) {
  float acc[MFT_LMAX] = {0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < MFT_F; ++j) {
    const float xv = xr[j];
#pragma unroll
    for (int l = 0; l < MFT_LMAX; ++l)
      if (l < L) acc[l] += wl[l][j] * xv;
  }
#pragma unroll
  for (int l = 0; l < MFT_LMAX; ++l) out[l] = acc[l];
}

static __global__ __launch_bounds__(256) void mft_tokpool_fwd(int HW, int L, const float* __restrict__ X, long ldx,
                                                              const float* __restrict__ wA,
                                                              const float* __restrict__ wV,
                                                              const float* __restrict__ add, float* __restrict__ A,
                                                              float* __restrict__ U, float* __restrict__ T, long ldt,
                                                              long strideT) {
  __shared__ float sA[MFT_LMAX][MFT_HW_MAX];
  __shared__ float sU[MFT_LMAX][MFT_F];
  __shared__ float swA[MFT_LMAX][MFT_F];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* Xb = X + (long)b * HW * ldx;
  if (tid < L * MFT_F) swA[tid >> 6][tid & 63] = wA[tid];
  __syncthreads();
  for (int i = tid; i < HW; i += 256) {
    float s[MFT_LMAX];
    tok_dots(Xb + (long)i * ldx, swA, L, s);
#pragma unroll
    for (int l = 0; l < MFT_LMAX; ++l)
      if (l < L) sA[l][i] = s[l];
  }
  __syncthreads();
  const int l = tid >> 6, lane = tid & 63;
  if (l < L) {   // wave-uniform
    float m = -INFINITY;
    for (int i = lane; i < HW; i += 64) m = fmaxf(m, sA[l][i]);
    m = wave_max(m);
    float z = 0.f;
    for (int i = lane; i < HW; i += 64) {
      const float e = __expf(sA[l][i] - m);
      sA[l][i] = e;
      z += e;
    }
    z = wave_sum(z);
    const float inv = 1.f / z;
    for (int i = lane; i < HW; i += 64) {
      const float a = sA[l][i] * inv;
      sA[l][i] = a;
      A[((long)b * L + l) * HW + i] = a;
    }
  }
  __syncthreads();
  if (l < L) {
    float acc = 0.f;
    for (int i = 0; i < HW; ++i) acc += sA[l][i] * Xb[(long)i * ldx + lane];
    sU[l][lane] = acc;
    U[((long)b * L + l) * MFT_F + lane] = acc;
  }
  __syncthreads();
  if (l < L) {
    float acc = 0.f;
    for (int j = 0; j < MFT_F; ++j) acc += sU[l][j] * wV[j * MFT_F + lane];
    if (add) acc += add[l * MFT_F + lane];
    T[(long)b * strideT + (long)l * ldt + lane] = acc;
  }
}

// part[b][l*64 + j] = dwA partial, part[b][L*64 + j*64 + k] = dwV partial
static __global__ __launch_bounds__(256) void mft_tokpool_bwd(int HW, int L, const float* __restrict__ X, long ldx,
                                                              const float* __restrict__ wA,
                                                              const float* __restrict__ wV,
                                                              const float* __restrict__ A, const float* __restrict__ U,
                                                              const float* __restrict__ dT, long ldt, long strideT,
                                                              float* __restrict__ dX, long lddx,
                                                              float* __restrict__ part) {
  __shared__ float sA[MFT_LMAX][MFT_HW_MAX];
  __shared__ float sdS[MFT_LMAX][MFT_HW_MAX];
  __shared__ float sdT[MFT_LMAX][MFT_F];
  __shared__ float sdU[MFT_LMAX][MFT_F];
  __shared__ float sU[MFT_LMAX][MFT_F];
  __shared__ float swA[MFT_LMAX][MFT_F];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int l = tid >> 6, lane = tid & 63;
  const float* Xb = X + (long)b * HW * ldx;
  if (l < L) {
    swA[l][lane] = wA[tid];
    sdT[l][lane] = dT[(long)b * strideT + (long)l * ldt + lane];
    sU[l][lane] = U[((long)b * L + l) * MFT_F + lane];
    for (int i = lane; i < HW; i += 64) sA[l][i] = A[((long)b * L + l) * HW + i];
  }
  __syncthreads();
  if (l < L) {   // dU[l][j] = sum_k dT[l][k] wV[j][k]
    float acc = 0.f;
    for (int k = 0; k < MFT_F; ++k) acc += sdT[l][k] * wV[lane * MFT_F + k];
    sdU[l][lane] = acc;
  }
  __syncthreads();
  for (int i = tid; i < HW; i += 256) {   // dA[l][i] = sum_j dU[l][j] X[i][j]
    float s[MFT_LMAX];
    tok_dots(Xb + (long)i * ldx, sdU, L, s);
#pragma unroll
    for (int ll = 0; ll < MFT_LMAX; ++ll)
      if (ll < L) sdS[ll][i] = s[ll];
  }
  __syncthreads();
  if (l < L) {   // dS = A (dA - sum_i A dA)
    float r = 0.f;
    for (int i = lane; i < HW; i += 64) r += sA[l][i] * sdS[l][i];
    r = wave_sum(r);
    for (int i = lane; i < HW; i += 64) sdS[l][i] = sA[l][i] * (sdS[l][i] - r);
  }
  __syncthreads();
  for (int e = tid; e < HW * MFT_F; e += 256) {   // dX[i][j] = sum_l A[l][i] dU[l][j] + dS[l][i] wA[l][j]
    const int i = e >> 6, j = e & 63;
    float acc = 0.f;
#pragma unroll
    for (int ll = 0; ll < MFT_LMAX; ++ll)
      if (ll < L) acc += sA[ll][i] * sdU[ll][j] + sdS[ll][i] * swA[ll][j];
    dX[((long)b * HW + i) * lddx + j] = acc;
  }
  float* pb = part + (long)b * (L * MFT_F + MFT_F * MFT_F);
  if (l < L) {   // dwA[l][j] = sum_i dS[l][i] X[i][j]
    float acc = 0.f;
    for (int i = 0; i < HW; ++i) acc += sdS[l][i] * Xb[(long)i * ldx + lane];
    pb[l * MFT_F + lane] = acc;
  }
  for (int e = tid; e < MFT_F * MFT_F; e += 256) {   // dwV[j][k] = sum_l U[l][j] dT[l][k]
    const int j = e >> 6, k = e & 63;
    float acc = 0.f;
#pragma unroll
    for (int ll = 0; ll < MFT_LMAX; ++ll)
      if (ll < L) acc += sU[ll][j] * sdT[ll][k];
    pb[L * MFT_F + e] = acc;
  }
}

static inline bool tok_ok(int B, int HW, int L, long ldx) {
  return B > 0 && B <= 65535 && HW > 0 && HW <= MFT_HW_MAX && L >= 1 && L <= MFT_LMAX && ldx >= MFT_F &&
         (long)B * HW * ldx < (1L << 31);
}

VC_API int vc_mft_tokpool_fwd(int B, int HW, int L, const float* X, long ldx, const float* wA, const float* wV,
                              const float* add, float* A, float* U, float* T, long ldt, long strideT,
                              hipStream_t stream) {
  VC_REQUIRE(tok_ok(B, HW, L, ldx));
  VC_REQUIRE(ldt >= MFT_F && strideT >= (long)L * ldt);
  VC_REQUIRE(X && wA && wV && A && U && T);
  hipLaunchKernelGGL(mft_tokpool_fwd, dim3(B), dim3(256), 0, stream, HW, L, X, ldx, wA, wV, add, A, U, T, ldt, strideT);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

VC_API int vc_mft_tokpool_bwd(int B, int HW, int L, const float* X, long ldx, const float* wA, const float* wV,
                              const float* A, const float* U, const float* dT, long ldt, long strideT, float* dX,
                              long lddx, float* dwA, float* dwV, float* ws, long ws_floats, hipStream_t stream) {
  VC_REQUIRE(tok_ok(B, HW, L, ldx));
  VC_REQUIRE(ldt >= MFT_F && strideT >= (long)L * ldt && lddx >= MFT_F && (long)B * HW * lddx < (1L << 31));
  const long ps = (long)L * MFT_F + MFT_F * MFT_F;
  VC_REQUIRE(ws && (long)B * ps <= ws_floats);
  VC_REQUIRE(X && wA && wV && A && U && dT && dX && dwA && dwV);
  hipLaunchKernelGGL(mft_tokpool_bwd, dim3(B), dim3(256), 0, stream, HW, L, X, ldx, wA, wV, A, U, dT, ldt, strideT, dX,
                     lddx, ws);
  VC_CHECK_LAUNCH();
  int rc = launch_sum_rows(B, L * MFT_F, ws, ps, 0, dwA, 0.f, stream);
  if (rc) return rc;
  return launch_sum_rows(B, MFT_F * MFT_F, ws, ps, (long)L * MFT_F, dwV, 0.f, stream);
}

// ---------------------------------------------------------------- MCrossAttention core
// One wave per (sample, head): lane e owns output feature e of the head's 64-wide q / k / v.
__device__ __forceinline__ void load8(const float* __restrict__ p, float (&v)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
}

__device__ __forceinline__ float dot8(const float (&a)[8], const float (&b)[8]) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) s += a[i] * b[i];
  return s;
}

// q, k[t], v[t] of lane e and the softmax weights a[t] (every lane holds all of them)
__device__ __forceinline__ void xattn_core(int T, const float* __restrict__ Yb, int h, const float (&wqe)[8],
                                           const float (&wke)[8], const float (&wve)[8], float scale, float& q,
                                           float (&k)[MFT_TMAX], float (&v)[MFT_TMAX], float (&a)[MFT_TMAX]) {
  float y[8];
  load8(Yb + h * 8, y);
  q = dot8(wqe, y);
  float m = -INFINITY;
#pragma unroll
  for (int t = 0; t < MFT_TMAX; ++t) {
    k[t] = v[t] = a[t] = 0.f;
    if (t < T) {
      load8(Yb + t * MFT_F + h * 8, y);
      k[t] = dot8(wke, y);
      v[t] = dot8(wve, y);
      a[t] = wave_sum(q * k[t]) * scale;
      m = fmaxf(m, a[t]);
    }
  }
  float z = 0.f;
#pragma unroll
  for (int t = 0; t < MFT_TMAX; ++t)
    if (t < T) {
      a[t] = __expf(a[t] - m);
      z += a[t];
    }
  const float inv = 1.f / z;
#pragma unroll
  for (int t = 0; t < MFT_TMAX; ++t) a[t] *= inv;
}

static __global__ __launch_bounds__(64) void mft_xattn_fwd(int T, const float* __restrict__ Y,
                                                           const float* __restrict__ wq, const float* __restrict__ wk,
                                                           const float* __restrict__ wv, float scale,
                                                           float* __restrict__ O, float* __restrict__ attn) {
  const int h = blockIdx.x, b = blockIdx.y, e = threadIdx.x;
  float wqe[8], wke[8], wve[8], q, k[MFT_TMAX], v[MFT_TMAX], a[MFT_TMAX];
  load8(wq + e * 8, wqe);
  load8(wk + e * 8, wke);
  load8(wv + e * 8, wve);
  xattn_core(T, Y + (long)b * T * MFT_F, h, wqe, wke, wve, scale, q, k, v, a);
  float o = 0.f;
#pragma unroll
  for (int t = 0; t < MFT_TMAX; ++t)
    if (t < T) {
      o += a[t] * v[t];
      if (e == 0) attn[((long)b * MFT_HEADS + h) * T + t] = a[t];
    }
  O[(long)b * (MFT_HEADS * MFT_F) + h * MFT_F + e] = o;
}

// one wave per sample, the heads in turn: lane e accumulates rows e of the three weight gradients over the heads
// (part[b][3][64][8]); q / k / v and the softmax are recomputed (a few hundred FMAs per lane)
static __global__ __launch_bounds__(64) void mft_xattn_bwd(int T, const float* __restrict__ Y,
                                                           const float* __restrict__ wq, const float* __restrict__ wk,
                                                           const float* __restrict__ wv, const float* __restrict__ dO,
                                                           float scale, float* __restrict__ dY,
                                                           float* __restrict__ part) {
  const int b = blockIdx.x, e = threadIdx.x;
  const float* Yb = Y + (long)b * T * MFT_F;
  float wqe[8], wke[8], wve[8];
  load8(wq + e * 8, wqe);
  load8(wk + e * 8, wke);
  load8(wv + e * 8, wve);
  float gq[8], gk[8], gv[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) gq[i] = gk[i] = gv[i] = 0.f;
  for (int h = 0; h < MFT_HEADS; ++h) {
    float q, k[MFT_TMAX], v[MFT_TMAX], a[MFT_TMAX];
    xattn_core(T, Yb, h, wqe, wke, wve, scale, q, k, v, a);
    const float doe = dO[(long)b * (MFT_HEADS * MFT_F) + h * MFT_F + e];
    float da[MFT_TMAX], r = 0.f;
#pragma unroll
    for (int t = 0; t < MFT_TMAX; ++t) {
      da[t] = 0.f;
      if (t < T) {
        da[t] = wave_sum(doe * v[t]);
        r += a[t] * da[t];
      }
    }
    float dq = 0.f, row0[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) row0[i] = 0.f;
#pragma unroll
    for (int t = 0; t < MFT_TMAX; ++t) {
      if (t < T) {
        const float ds = a[t] * (da[t] - r) * scale;   // d(score before the scale)
        const float dk = ds * q, dv = a[t] * doe;
        dq += ds * k[t];
        float y[8];
        load8(Yb + t * MFT_F + h * 8, y);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          gk[i] += dk * y[i];
          gv[i] += dv * y[i];
          const float s = wave_sum(dk * wke[i] + dv * wve[i]);
          if (t == 0)
            row0[i] = s;   // row 0 also takes the query's share, known only after this loop (dq)
          else if (e == i)
            dY[((long)b * T + t) * MFT_F + h * 8 + i] = s;
        }
      }
    }
    {
      float y0[8];
      load8(Yb + h * 8, y0);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        gq[i] += dq * y0[i];
        const float s = wave_sum(dq * wqe[i]) + row0[i];
        if (e == i) dY[(long)b * T * MFT_F + h * 8 + i] = s;
      }
    }
  }
  float* pb = part + (long)b * (3 * MFT_F * 8);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    pb[e * 8 + i] = gq[i];
    pb[512 + e * 8 + i] = gk[i];
    pb[1024 + e * 8 + i] = gv[i];
  }
}

static inline bool xattn_ok(int B, int T) { return B > 0 && B <= 65535 && T >= 2 && T <= MFT_TMAX; }

VC_API int vc_mft_xattn_fwd(int B, int T, const float* Y, const float* wq, const float* wk, const float* wv,
                            float scale, float* O, float* attn, hipStream_t stream) {
  VC_REQUIRE(xattn_ok(B, T));
  VC_REQUIRE(Y && wq && wk && wv && O && attn);
  VC_REQUIRE((((uintptr_t)Y | (uintptr_t)wq | (uintptr_t)wk | (uintptr_t)wv) & 15) == 0);
  hipLaunchKernelGGL(mft_xattn_fwd, dim3(MFT_HEADS, B), dim3(64), 0, stream, T, Y, wq, wk, wv, scale, O, attn);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

VC_API int vc_mft_xattn_bwd(int B, int T, const float* Y, const float* wq, const float* wk, const float* wv,
                            const float* attn, const float* dO, float scale, float* dY, float* dwq, float* dwk,
                            float* dwv, float* ws, long ws_floats, hipStream_t stream) {
  VC_REQUIRE(xattn_ok(B, T));
  VC_REQUIRE(Y && wq && wk && wv && dO && dY && dwq && dwk && dwv);
  VC_REQUIRE((((uintptr_t)Y | (uintptr_t)wq | (uintptr_t)wk | (uintptr_t)wv) & 15) == 0);
  const long ps = 3 * MFT_F * 8;
  VC_REQUIRE(ws && (long)B * ps <= ws_floats);
  (void)attn;   // the softmax is recomputed with the forward's own arithmetic; attn is the forward's record
  hipLaunchKernelGGL(mft_xattn_bwd, dim3(B), dim3(64), 0, stream, T, Y, wq, wk, wv, dO, scale, dY, ws);
  VC_CHECK_LAUNCH();
  int rc = launch_sum_rows(B, 512, ws, ps, 0, dwq, 0.f, stream);
  if (rc) return rc;
  rc = launch_sum_rows(B, 512, ws, ps, 512, dwk, 0.f, stream);
  if (rc) return rc;
  return launch_sum_rows(B, 512, ws, ps, 1024, dwv, 0.f, stream);
}

// ---------------------------------------------------------------- broadcast residual
static __global__ void mft_bcast_add_fwd(int n, int T, int D, const float* __restrict__ h, const float* __restrict__ a,
                                         float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int d = i % D, b = i / (T * D);
  out[i] = h[i] + a[b * D + d];
}

static __global__ void mft_bcast_add_bwd(int n, int T, int D, const float* __restrict__ dout, float* __restrict__ da) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int d = i % D, b = i / D;
  float acc = 0.f;
  for (int t = 0; t < T; ++t) acc += dout[((long)b * T + t) * D + d];
  da[i] = acc;
}

VC_API int vc_mft_bcast_add_fwd(int B, int T, int D, const float* h, const float* a, float* out, hipStream_t stream) {
  VC_REQUIRE(B > 0 && T > 0 && D > 0 && h && a && out);
  VC_REQUIRE_I32((long)B * T * D);
  const int n = B * T * D;
  hipLaunchKernelGGL(mft_bcast_add_fwd, dim3(vc_cdiv(n, 256)), dim3(256), 0, stream, n, T, D, h, a, out);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

VC_API int vc_mft_bcast_add_bwd(int B, int T, int D, const float* dout, float* da, hipStream_t stream) {
  VC_REQUIRE(B > 0 && T > 0 && D > 0 && dout && da);
  VC_REQUIRE_I32((long)B * T * D);
  const int n = B * D;
  hipLaunchKernelGGL(mft_bcast_add_bwd, dim3(vc_cdiv(n, 256)), dim3(256), 0, stream, n, T, D, dout, da);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

// ---------------------------------------------------------------- Adam with coupled L2 weight decay
// step[0] = t (incremented), step[1] = 1 - beta1^t, step[2] = sqrt(1 - beta2^t)  (vc_adamw's layout)
static __global__ void mft_adam_step_inc(float* step, const float* __restrict__ hyper) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const float t = step[0] + 1.f;
    step[0] = t;
    step[1] = 1.f - powf(hyper[1], t);
    step[2] = sqrtf(1.f - powf(hyper[2], t));
  }
}

struct AdamL2Hyper {
  float lr, b1, b2, eps, wd, gs, bc1, sbc2;
};

__device__ __forceinline__ void adam_l2_elem(const AdamL2Hyper& h, float& p, float g, float& m, float& v) {
  const float gi = g * h.gs + h.wd * p;
  m = m + (gi - m) * (1.f - h.b1);
  v = v * h.b2 + (1.f - h.b2) * gi * gi;
  const float denom = sqrtf(v) / h.sbc2 + h.eps;
  p = p - (h.lr / h.bc1) * (m / denom);
}

// 4 elements per thread (16-B loads / stores) over [0, n4 * 4), a scalar tail after
static __global__ void mft_adam(long n, float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                float* __restrict__ v, const float* __restrict__ hyper,
                                const float* __restrict__ step) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const AdamL2Hyper h{hyper[0], hyper[1], hyper[2], hyper[3], hyper[4], hyper[5], step[1], step[2]};
  const long n4 = n >> 2;
  if (i < n4) {
    float4 pv = reinterpret_cast<float4*>(p)[i];
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    float4 mv = reinterpret_cast<float4*>(m)[i];
    float4 vv = reinterpret_cast<float4*>(v)[i];
    adam_l2_elem(h, pv.x, gv.x, mv.x, vv.x);
    adam_l2_elem(h, pv.y, gv.y, mv.y, vv.y);
    adam_l2_elem(h, pv.z, gv.z, mv.z, vv.z);
    adam_l2_elem(h, pv.w, gv.w, mv.w, vv.w);
    reinterpret_cast<float4*>(p)[i] = pv;
    reinterpret_cast<float4*>(m)[i] = mv;
    reinterpret_cast<float4*>(v)[i] = vv;
  } else {
    const long j = n4 * 4 + (i - n4);
    if (j < n) adam_l2_elem(h, p[j], g[j], m[j], v[j]);
  }
}

VC_API int vc_adam(long n, float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const float* hyper,
                   float* step, hipStream_t stream) {
  VC_REQUIRE(n >= 0);
  VC_REQUIRE(((uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) % 16 == 0);
  hipLaunchKernelGGL(mft_adam_step_inc, dim3(1), dim3(64), 0, stream, step, hyper);
  VC_CHECK_LAUNCH();
  if (n == 0) return VC_OK;
  const long threads = (n >> 2) + (n & 3);
  hipLaunchKernelGGL(mft_adam, dim3(vc_cdiv(threads, 256)), dim3(256), 0, stream, n, params, grads, exp_avg, exp_avg_sq,
                     hyper, step);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

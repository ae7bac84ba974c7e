// HCTnet comparison model (model/compare_method/HCTnet.py): the ops no other model has.
//   vc_hct_tokpool_fwd / _bwd    the tokeniser for L <= 8 tokens: softmax-over-pixels pooling written into rows 1..L of
//                                a [B, L+1, 64] token buffer, the cls row, the position rows and the embedding dropout
//   vc_hct_encoder_fwd / _bwd    one whole pre-norm encoder layer of a [B, T, 64] sequence (T <= 9), both branches in
//                                one launch; a block owns one sample's sequence in LDS
//   vc_hct_ctattn_fwd / _bwd     the cross-token step (LayerNorm of the cls row, single-query 8 x 64 attention over the
//                                other branch's patch tokens, to_out, residual), both directions in one launch
// All fp32 with fp32 accumulation, no atomics: every weight gradient is a per-sample partial row in ws, summed by
// launch_sum_rows in a fixed order, so two runs give the same bits.  Both backwards recompute the forward's
// intermediates from the saved input (a few hundred kFLOP per sample) with the forward's own code.
#include "common.h"

#define HCT_F 64
#define HCT_LMAX 8
#define HCT_TMAX 9
#define HCT_HW_MAX 784      // (30 - 2)^2: the LiDAR map of a 30 x 30 patch
#define HCT_LN_EPS 1e-5f

// s2eft.hip's dropout hash (vc_dropout_fwd): keep_i = u_i >= p with u_i = hash(seed, i) / 2^24
__device__ __forceinline__ bool hct_keep(unsigned long long seed, uint32_t i, float p) {
  uint64_t z = seed ^ ((uint64_t)i * 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  const uint32_t h = (uint32_t)((z ^ (z >> 31)) >> 32);
  return (float)(h >> 8) * (1.0f / 16777216.0f) >= p;
}

// One dropout site of a block.  gen: the keep decision is drawn (element index base + i of the whole mask buffer) and
// stored; otherwise it is read back.  p == 0 keeps everything and touches no mask.
struct HctDrop {
  unsigned char* mk;   // this block's mask bytes of the site (null only with p == 0)
  uint32_t base;       // index of mk[0] in the whole mask buffer (the hash counter)
  float p, scale;
  unsigned long long seed;
  bool gen;
  __device__ __forceinline__ float apply(int i, float v) const {
    if (p <= 0.f) {
      if (gen && mk) mk[i] = 1;
      return v;
    }
    bool keep;
    if (gen) {
      keep = hct_keep(seed, base + (uint32_t)i, p);
      mk[i] = keep ? 1 : 0;
    } else {
      keep = mk[i] != 0;
    }
    return keep ? v * scale : 0.f;
  }
};

__device__ __forceinline__ HctDrop hct_drop(unsigned char* mask, long off, float p, unsigned long long seed, bool gen) {
  HctDrop d;
  d.mk = mask ? mask + off : nullptr;
  d.base = (uint32_t)off;
  d.p = p;
  d.scale = p > 0.f ? 1.0f / (1.0f - p) : 1.f;
  d.seed = seed;
  d.gen = gen;
  return d;
}

__device__ __forceinline__ float hct_gelu(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752f)); }
__device__ __forceinline__ float hct_gelu_grad(float x) {
  return 0.5f * (1.f + erff(x * 0.70710678118654752f)) + x * 0.3989422804014327f * __expf(-0.5f * x * x);
}

// ---------------------------------------------------------------- tokeniser
// One block (512 threads = 8 waves) per sample; wave l owns token l's softmax.
__device__ __forceinline__ void hct_tok_dots(const float* __restrict__ xr, const float (*wl)[HCT_F], int L, float* out) {
  float acc[HCT_LMAX];
#pragma unroll
  for (int l = 0; l < HCT_LMAX; ++l) acc[l] = 0.f;
  for (int j = 0; j < HCT_F; ++j) {
    const float xv = xr[j];
#pragma unroll
    for (int l = 0; l < HCT_LMAX; ++l)
      if (l < L) acc[l] += wl[l][j] * xv;
  }
#pragma unroll
  for (int l = 0; l < HCT_LMAX; ++l) out[l] = acc[l];
}

static __global__ __launch_bounds__(512) void hct_tokpool_fwd(int HW, int L, const float* __restrict__ X, long ldx,
                                                              const float* __restrict__ wA,
                                                              const float* __restrict__ wV,
                                                              const float* __restrict__ cls,
                                                              const float* __restrict__ pos, float p,
                                                              unsigned long long seed,
                                                              const unsigned long long* __restrict__ seed_dev,
                                                              float* __restrict__ A, float* __restrict__ U,
                                                              float* __restrict__ T,
                                                              unsigned char* __restrict__ mask) {
  __shared__ float sA[HCT_LMAX][HCT_HW_MAX];
  __shared__ float sU[HCT_LMAX][HCT_F];
  __shared__ float swA[HCT_LMAX][HCT_F];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* Xb = X + (long)b * HW * ldx;
  const long tb = (long)b * (L + 1) * HCT_F;
  const HctDrop dr = hct_drop(mask, tb, p, vc_site_seed(seed, seed_dev), true);
  if (tid < L * HCT_F) swA[tid >> 6][tid & 63] = wA[tid];
  __syncthreads();
  for (int i = tid; i < HW; i += 512) {
    float s[HCT_LMAX];
    hct_tok_dots(Xb + (long)i * ldx, swA, L, s);
#pragma unroll
    for (int l = 0; l < HCT_LMAX; ++l)
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
    U[((long)b * L + l) * HCT_F + lane] = acc;
  }
  __syncthreads();
  if (l < L) {
    float acc = 0.f;
    for (int j = 0; j < HCT_F; ++j) acc += sU[l][j] * wV[j * HCT_F + lane];
    acc += pos[(l + 1) * HCT_F + lane];
    T[tb + (l + 1) * HCT_F + lane] = dr.apply((l + 1) * HCT_F + lane, acc);
  }
  if (tid < HCT_F) T[tb + tid] = dr.apply(tid, cls[tid] + pos[tid]);
}

// part[b] = [L*64 dwA | 64*64 dwV | (L+1)*64 dpos]: this sample's partial sums
static __global__ __launch_bounds__(512) void hct_tokpool_bwd(int HW, int L, const float* __restrict__ X, long ldx,
                                                              const float* __restrict__ wA,
                                                              const float* __restrict__ wV,
                                                              const float* __restrict__ A, const float* __restrict__ U,
                                                              const float* __restrict__ dT,
                                                              const unsigned char* __restrict__ mask, float p,
                                                              float* __restrict__ dX, long lddx,
                                                              float* __restrict__ part) {
  __shared__ float sA[HCT_LMAX][HCT_HW_MAX];
  __shared__ float sdS[HCT_LMAX][HCT_HW_MAX];
  __shared__ float sdT[HCT_LMAX + 1][HCT_F];
  __shared__ float sdU[HCT_LMAX][HCT_F];
  __shared__ float sU[HCT_LMAX][HCT_F];
  __shared__ float swA[HCT_LMAX][HCT_F];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int l = tid >> 6, lane = tid & 63;
  const float* Xb = X + (long)b * HW * ldx;
  const long tb = (long)b * (L + 1) * HCT_F;
  const HctDrop dr = hct_drop(const_cast<unsigned char*>(mask), tb, p, 0, false);
  const long ps = (long)L * HCT_F + HCT_F * HCT_F + (long)(L + 1) * HCT_F;
  float* pb = part + (long)b * ps;
  for (int e = tid; e < (L + 1) * HCT_F; e += 512) {   // the embedding dropout's backward; dpos partial = this row
    const float g = dr.apply(e, dT[tb + e]);
    sdT[e >> 6][e & 63] = g;
    pb[L * HCT_F + HCT_F * HCT_F + e] = g;
  }
  if (l < L) {
    swA[l][lane] = wA[tid];
    sU[l][lane] = U[((long)b * L + l) * HCT_F + lane];
    for (int i = lane; i < HW; i += 64) sA[l][i] = A[((long)b * L + l) * HW + i];
  }
  __syncthreads();
  if (l < L) {   // dU[l][j] = sum_k dT[l+1][k] wV[j][k]
    float acc = 0.f;
    for (int k = 0; k < HCT_F; ++k) acc += sdT[l + 1][k] * wV[lane * HCT_F + k];
    sdU[l][lane] = acc;
  }
  __syncthreads();
  for (int i = tid; i < HW; i += 512) {   // dA[l][i] = sum_j dU[l][j] X[i][j]
    float s[HCT_LMAX];
    hct_tok_dots(Xb + (long)i * ldx, sdU, L, s);
#pragma unroll
    for (int ll = 0; ll < HCT_LMAX; ++ll)
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
  for (int e = tid; e < HW * HCT_F; e += 512) {   // dX[i][j] = sum_l A[l][i] dU[l][j] + dS[l][i] wA[l][j]
    const int i = e >> 6, j = e & 63;
    float acc = 0.f;
#pragma unroll
    for (int ll = 0; ll < HCT_LMAX; ++ll)
      if (ll < L) acc += sA[ll][i] * sdU[ll][j] + sdS[ll][i] * swA[ll][j];
    dX[((long)b * HW + i) * lddx + j] = acc;
  }
  if (l < L) {   // dwA[l][j] = sum_i dS[l][i] X[i][j]
    float acc = 0.f;
    for (int i = 0; i < HW; ++i) acc += sdS[l][i] * Xb[(long)i * ldx + lane];
    pb[l * HCT_F + lane] = acc;
  }
  for (int e = tid; e < HCT_F * HCT_F; e += 512) {   // dwV[j][k] = sum_l U[l][j] dT[l+1][k]
    const int j = e >> 6, k = e & 63;
    float acc = 0.f;
#pragma unroll
    for (int ll = 0; ll < HCT_LMAX; ++ll)
      if (ll < L) acc += sU[ll][j] * sdT[ll + 1][k];
    pb[L * HCT_F + e] = acc;
  }
}

static inline bool hct_tok_ok(int B, int HW, int L, long ldx) {
  return B > 0 && B <= 65535 && HW > 0 && HW <= HCT_HW_MAX && L >= 1 && L <= HCT_LMAX && ldx >= HCT_F &&
         (long)B * HW * ldx < (1L << 31);
}

static int hct_tokpool_fwd_launch(int B, int HW, int L, const float* X, long ldx, const float* wA, const float* wV,
                                  const float* cls, const float* pos, float p, unsigned long long seed,
                                  const unsigned long long* seed_dev, float* A, float* U, float* T,
                                  unsigned char* mask, hipStream_t stream) {
  VC_REQUIRE(hct_tok_ok(B, HW, L, ldx));
  VC_REQUIRE(p >= 0.f && p < 1.f && (p == 0.f || mask));
  VC_REQUIRE(X && wA && wV && cls && pos && A && U && T);
  hipLaunchKernelGGL(hct_tokpool_fwd, dim3(B), dim3(512), 0, stream, HW, L, X, ldx, wA, wV, cls, pos, p, seed,
                     seed_dev, A, U, T, mask);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

VC_API int vc_hct_tokpool_fwd(int B, int HW, int L, const float* X, long ldx, const float* wA, const float* wV,
                              const float* cls, const float* pos, float p, unsigned long long seed, float* A, float* U,
                              float* T, unsigned char* mask, hipStream_t stream) {
  return hct_tokpool_fwd_launch(B, HW, L, X, ldx, wA, wV, cls, pos, p, seed, nullptr, A, U, T, mask, stream);
}

VC_API int vc_hct_tokpool_fwd_ds(int B, int HW, int L, const float* X, long ldx, const float* wA, const float* wV,
                                 const float* cls, const float* pos, float p, const unsigned long long* seed_dev,
                                 unsigned long long site_offset, float* A, float* U, float* T, unsigned char* mask,
                                 hipStream_t stream) {
  VC_REQUIRE(seed_dev);
  return hct_tokpool_fwd_launch(B, HW, L, X, ldx, wA, wV, cls, pos, p, site_offset, seed_dev, A, U, T, mask, stream);
}

VC_API int vc_hct_tokpool_bwd(int B, int HW, int L, const float* X, long ldx, const float* wA, const float* wV,
                              const float* A, const float* U, const float* dT, const unsigned char* mask, float p,
                              float* dX, long lddx, float* ws, long ws_floats, int row0, float* dwA, float* dwV,
                              float* dpos, float* dcls, hipStream_t stream) {
  VC_REQUIRE(hct_tok_ok(B, HW, L, ldx));
  VC_REQUIRE(p >= 0.f && p < 1.f && (p == 0.f || mask));
  VC_REQUIRE(lddx >= HCT_F && (long)B * HW * lddx < (1L << 31) && row0 >= 0 && row0 <= 65535);
  const long ps = (long)L * HCT_F + HCT_F * HCT_F + (long)(L + 1) * HCT_F;
  VC_REQUIRE(ws && ((long)row0 + B) * ps <= ws_floats);
  VC_REQUIRE(X && wA && wV && A && U && dT && dX);
  VC_REQUIRE((dwA && dwV && dpos && dcls) || (!dwA && !dwV && !dpos && !dcls));
  hipLaunchKernelGGL(hct_tokpool_bwd, dim3(B), dim3(512), 0, stream, HW, L, X, ldx, wA, wV, A, U, dT, mask, p, dX, lddx,
                     ws + (long)row0 * ps);
  VC_CHECK_LAUNCH();
  if (!dwA) return VC_OK;
  const int R = row0 + B;
  const long opos = (long)L * HCT_F + HCT_F * HCT_F;
  int rc = launch_sum_rows(R, L * HCT_F, ws, ps, 0, dwA, 0.f, stream);
  if (rc) return rc;
  rc = launch_sum_rows(R, HCT_F * HCT_F, ws, ps, (long)L * HCT_F, dwV, 0.f, stream);
  if (rc) return rc;
  rc = launch_sum_rows(R, (L + 1) * HCT_F, ws, ps, opos, dpos, 0.f, stream);
  if (rc) return rc;
  return launch_sum_rows(R, HCT_F, ws, ps, opos, dcls, 0.f, stream);
}

// ---------------------------------------------------------------- encoder layer
// the packed weights of one Transformer(dim 64, depth 1, heads 8, mlp_dim 8), in the module's parameter order
#define E_LN1W 0
#define E_LN1B 64
#define E_QKVW 128      // [192][64]
#define E_QKVB 12416
#define E_NN1W 12608    // [64][64]
#define E_NN1B 16704
#define E_LN2W 16768
#define E_LN2B 16832
#define E_FC1W 16896    // [8][64]
#define E_FC1B 17408
#define E_FC2W 17416    // [64][8]
#define E_FC2B 17928
#define E_SIZE VC_HCT_ENC_FLOATS
#define E_HEADS 8
#define E_HD 8
#define E_MLP 8
#define E_MASK (HCT_F + E_MLP + HCT_F)   // mask bytes per token row: attention output, hidden, MLP output

struct EncFwd {
  float x[HCT_TMAX * 64], xn[HCT_TMAX * 64], qkv[HCT_TMAX * 192], att[E_HEADS * HCT_TMAX * HCT_TMAX];
  float o[HCT_TMAX * 64], x2[HCT_TMAX * 64], xn2[HCT_TMAX * 64], h[HCT_TMAX * E_MLP], g[HCT_TMAX * E_MLP];
  float mu1[HCT_TMAX], rs1[HCT_TMAX], mu2[HCT_TMAX], rs2[HCT_TMAX];
};

// LayerNorm of rows x [T][64] -> y; wave w takes rows w, w + 4, ...
__device__ __forceinline__ void hct_ln_rows(int T, const float* x, const float* __restrict__ w,
                                            const float* __restrict__ b, float* y, float* mu, float* rs) {
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int t = wv; t < T; t += 4) {
    const float v = x[t * 64 + lane];
    const float mean = wave_sum(v) * (1.f / 64.f);
    const float d = v - mean;
    const float var = wave_sum(d * d) * (1.f / 64.f);
    const float r = 1.f / sqrtf(var + HCT_LN_EPS);
    y[t * 64 + lane] = d * r * w[lane] + b[lane];
    if (lane == 0) {
      mu[t] = mean;
      rs[t] = r;
    }
  }
}

// LayerNorm backward of rows: dx[t][k] (+)= rs (g - mean(g) - xhat mean(g xhat)), g = dy w; dw / db partial columns
__device__ __forceinline__ void hct_ln_rows_bwd(int T, const float* x, const float* dy, const float* __restrict__ w,
                                                const float* mu, const float* rs, float* dx, bool accumulate) {
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int t = wv; t < T; t += 4) {
    const float xh = (x[t * 64 + lane] - mu[t]) * rs[t];
    const float g = dy[t * 64 + lane] * w[lane];
    const float m1 = wave_sum(g) * (1.f / 64.f);
    const float m2 = wave_sum(g * xh) * (1.f / 64.f);
    const float v = rs[t] * (g - m1 - xh * m2);
    dx[t * 64 + lane] = accumulate ? dx[t * 64 + lane] + v : v;
  }
}

// y[t][n] = sum_k in[t][k] W[n][k] for this thread's column n = tid & 63 and rows t = tid >> 6, + 4, + 8 (K = 64)
__device__ __forceinline__ void hct_lin64(int T, const float* in, const float* __restrict__ W, float (&acc)[3]) {
  const int n = threadIdx.x & 63, tq = threadIdx.x >> 6;
  acc[0] = acc[1] = acc[2] = 0.f;
  const float4* wr = reinterpret_cast<const float4*>(W + n * 64);
  for (int k4 = 0; k4 < 16; ++k4) {
    const float4 w = wr[k4];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int t = tq + 4 * r;
      if (t < T) {
        const float* xp = in + t * 64 + k4 * 4;
        acc[r] += xp[0] * w.x + xp[1] * w.y + xp[2] * w.z + xp[3] * w.w;
      }
    }
  }
}

// the whole layer for one sample: fills s, returns through Y (nullable) the output rows
__device__ __forceinline__ void hct_enc_core(EncFwd& s, int T, const float* __restrict__ X, const float* __restrict__ W,
                                             const HctDrop& d0, const HctDrop& d1, const HctDrop& d2,
                                             float* __restrict__ Y) {
  const int tid = threadIdx.x;
  for (int e = tid; e < T * 64; e += 256) s.x[e] = X[e];
  __syncthreads();
  hct_ln_rows(T, s.x, W + E_LN1W, W + E_LN1B, s.xn, s.mu1, s.rs1);
  __syncthreads();
  if (tid < 192) {   // qkv[t][n] = b[n] + sum_k xn[t][k] Wqkv[n][k]
    float acc[HCT_TMAX];
    const float bv = W[E_QKVB + tid];
#pragma unroll
    for (int t = 0; t < HCT_TMAX; ++t) acc[t] = bv;
    const float4* wr = reinterpret_cast<const float4*>(W + E_QKVW + tid * 64);
    for (int k4 = 0; k4 < 16; ++k4) {
      const float4 w = wr[k4];
#pragma unroll
      for (int t = 0; t < HCT_TMAX; ++t)
        if (t < T) {
          const float* xp = s.xn + t * 64 + k4 * 4;
          acc[t] += xp[0] * w.x + xp[1] * w.y + xp[2] * w.z + xp[3] * w.w;
        }
    }
#pragma unroll
    for (int t = 0; t < HCT_TMAX; ++t)
      if (t < T) s.qkv[t * 192 + tid] = acc[t];
  }
  __syncthreads();
  for (int e = tid; e < E_HEADS * T * T; e += 256) {   // scores, scale = 64^-0.5 (the model width, HCTnet.py:61)
    const int j = e % T, i = (e / T) % T, h = e / (T * T);
    float acc = 0.f;
#pragma unroll
    for (int d = 0; d < E_HD; ++d) acc += s.qkv[i * 192 + h * E_HD + d] * s.qkv[j * 192 + 64 + h * E_HD + d];
    s.att[(h * HCT_TMAX + i) * HCT_TMAX + j] = acc * 0.125f;
  }
  __syncthreads();
  if (tid < E_HEADS * T) {
    const int i = tid % T, h = tid / T;
    float* a = s.att + (h * HCT_TMAX + i) * HCT_TMAX;
    float m = -INFINITY, z = 0.f;
    for (int j = 0; j < T; ++j) m = fmaxf(m, a[j]);
    for (int j = 0; j < T; ++j) {
      a[j] = __expf(a[j] - m);
      z += a[j];
    }
    const float inv = 1.f / z;
    for (int j = 0; j < T; ++j) a[j] *= inv;
  }
  __syncthreads();
  for (int e = tid; e < T * 64; e += 256) {   // o[i][h*8+d] = sum_j att[h][i][j] v[j][h*8+d]
    const int c = e & 63, i = e >> 6, h = c >> 3;
    float acc = 0.f;
    for (int j = 0; j < T; ++j) acc += s.att[(h * HCT_TMAX + i) * HCT_TMAX + j] * s.qkv[j * 192 + 128 + c];
    s.o[e] = acc;
  }
  __syncthreads();
  {
    float acc[3];
    hct_lin64(T, s.o, W + E_NN1W, acc);
    const int n = tid & 63, tq = tid >> 6;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int t = tq + 4 * r;
      if (t < T) s.x2[t * 64 + n] = s.x[t * 64 + n] + d0.apply(t * 64 + n, acc[r] + W[E_NN1B + n]);
    }
  }
  __syncthreads();
  hct_ln_rows(T, s.x2, W + E_LN2W, W + E_LN2B, s.xn2, s.mu2, s.rs2);
  __syncthreads();
  if (tid < T * E_MLP) {
    const int m = tid & 7, t = tid >> 3;
    float acc = W[E_FC1B + m];
    for (int k = 0; k < 64; ++k) acc += s.xn2[t * 64 + k] * W[E_FC1W + m * 64 + k];
    s.h[tid] = acc;
    s.g[tid] = d1.apply(tid, hct_gelu(acc));
  }
  __syncthreads();
  if (Y) {
    for (int e = tid; e < T * 64; e += 256) {
      const int n = e & 63, t = e >> 6;
      float acc = W[E_FC2B + n];
#pragma unroll
      for (int m = 0; m < E_MLP; ++m) acc += s.g[t * E_MLP + m] * W[E_FC2W + n * E_MLP + m];
      Y[e] = s.x2[e] + d2.apply(e, acc);
    }
  }
}

struct EncP {
  float pa, ph, po;
};

static __global__ __launch_bounds__(256) void hct_encoder_fwd(int B, int T, const float* __restrict__ X, long strideX,
                                                              const float* __restrict__ W0,
                                                              const float* __restrict__ W1, EncP p0, EncP p1,
                                                              unsigned long long seed,
                                                              const unsigned long long* __restrict__ seed_dev,
                                                              float* __restrict__ Y, long strideY,
                                                              unsigned char* __restrict__ mask) {
  __shared__ EncFwd s;
  seed = vc_site_seed(seed, seed_dev);
  const int b = blockIdx.x, br = blockIdx.y;
  const float* W = br ? W1 : W0;
  const EncP p = br ? p1 : p0;
  const long mb = ((long)br * B + b) * T * E_MASK;
  const HctDrop d0 = hct_drop(mask, mb, p.pa, seed, true);
  const HctDrop d1 = hct_drop(mask, mb + T * 64, p.ph, seed, true);
  const HctDrop d2 = hct_drop(mask, mb + T * (64 + E_MLP), p.po, seed, true);
  hct_enc_core(s, T, X + br * strideX + (long)b * T * 64, W, d0, d1, d2, Y + br * strideY + (long)b * T * 64);
}

// dW[n][k] = sum_t dy[t][n] in[t][k] over this block's rows, written to the partial row
__device__ __forceinline__ void hct_outer(int T, int N, int K, int lddy, const float* dy, int ldin, const float* in,
                                          float* __restrict__ out) {
  for (int e = threadIdx.x; e < N * K; e += 256) {
    const int n = e / K, k = e - n * K;
    float acc = 0.f;
    for (int t = 0; t < T; ++t) acc += dy[t * lddy + n] * in[t * ldin + k];
    out[e] = acc;
  }
}

__device__ __forceinline__ void hct_colsum(int T, int N, int ld, const float* dy, float* __restrict__ out) {
  for (int n = threadIdx.x; n < N; n += 256) {
    float acc = 0.f;
    for (int t = 0; t < T; ++t) acc += dy[t * ld + n];
    out[n] = acc;
  }
}

// dgamma[k] = sum_t dy[t][k] xhat[t][k], dbeta[k] = sum_t dy[t][k]
__device__ __forceinline__ void hct_ln_wgrad(int T, const float* x, const float* dy, const float* mu, const float* rs,
                                             float* __restrict__ dw, float* __restrict__ db) {
  if (threadIdx.x < 64) {
    const int k = threadIdx.x;
    float a = 0.f, c = 0.f;
    for (int t = 0; t < T; ++t) {
      const float g = dy[t * 64 + k];
      a += g * (x[t * 64 + k] - mu[t]) * rs[t];
      c += g;
    }
    dw[k] = a;
    db[k] = c;
  }
}

struct EncBwd {
  float df[HCT_TMAX * 64], dh[HCT_TMAX * E_MLP], dxn2[HCT_TMAX * 64], dx2[HCT_TMAX * 64], da1[HCT_TMAX * 64];
  float dO[HCT_TMAX * 64], datt[E_HEADS * HCT_TMAX * HCT_TMAX], dqkv[HCT_TMAX * 192], dxn[HCT_TMAX * 64];
};

static __global__ __launch_bounds__(256) void hct_encoder_bwd(int B, int T, const float* __restrict__ X, long strideX,
                                                              const float* __restrict__ W0,
                                                              const float* __restrict__ W1, EncP p0, EncP p1,
                                                              const unsigned char* __restrict__ mask,
                                                              const float* __restrict__ dY, long strideDY,
                                                              float* __restrict__ dX, long strideDX,
                                                              float* __restrict__ part) {
  __shared__ EncFwd s;
  __shared__ EncBwd g;
  const int b = blockIdx.x, br = blockIdx.y, tid = threadIdx.x;
  const float* W = br ? W1 : W0;
  const EncP p = br ? p1 : p0;
  const long mb = ((long)br * B + b) * T * E_MASK;
  unsigned char* mk = const_cast<unsigned char*>(mask);
  const HctDrop d0 = hct_drop(mk, mb, p.pa, 0, false);
  const HctDrop d1 = hct_drop(mk, mb + T * 64, p.ph, 0, false);
  const HctDrop d2 = hct_drop(mk, mb + T * (64 + E_MLP), p.po, 0, false);
  hct_enc_core(s, T, X + br * strideX + (long)b * T * 64, W, d0, d1, d2, nullptr);
  float* pb = part + ((long)br * B + b) * E_SIZE;
  const float* dYb = dY + br * strideDY + (long)b * T * 64;
  // MLP: y = x2 + drop2(fc2(drop1(gelu(fc1(LN2(x2))))))
  for (int e = tid; e < T * 64; e += 256) {
    const float v = dYb[e];
    g.dx2[e] = v;
    g.df[e] = d2.apply(e, v);
  }
  __syncthreads();
  hct_colsum(T, 64, 64, g.df, pb + E_FC2B);
  hct_outer(T, 64, E_MLP, 64, g.df, E_MLP, s.g, pb + E_FC2W);
  if (tid < T * E_MLP) {
    const int m = tid & 7, t = tid >> 3;
    float acc = 0.f;
    for (int n = 0; n < 64; ++n) acc += g.df[t * 64 + n] * W[E_FC2W + n * E_MLP + m];
    g.dh[tid] = d1.apply(tid, acc) * hct_gelu_grad(s.h[tid]);
  }
  __syncthreads();
  hct_colsum(T, E_MLP, E_MLP, g.dh, pb + E_FC1B);
  hct_outer(T, E_MLP, 64, E_MLP, g.dh, 64, s.xn2, pb + E_FC1W);
  for (int e = tid; e < T * 64; e += 256) {
    const int k = e & 63, t = e >> 6;
    float acc = 0.f;
#pragma unroll
    for (int m = 0; m < E_MLP; ++m) acc += g.dh[t * E_MLP + m] * W[E_FC1W + m * 64 + k];
    g.dxn2[e] = acc;
  }
  __syncthreads();
  hct_ln_wgrad(T, s.x2, g.dxn2, s.mu2, s.rs2, pb + E_LN2W, pb + E_LN2B);
  hct_ln_rows_bwd(T, s.x2, g.dxn2, W + E_LN2W, s.mu2, s.rs2, g.dx2, true);
  __syncthreads();
  // attention: x2 = x + drop0(nn1(o))
  for (int e = tid; e < T * 64; e += 256) g.da1[e] = d0.apply(e, g.dx2[e]);
  __syncthreads();
  hct_colsum(T, 64, 64, g.da1, pb + E_NN1B);
  hct_outer(T, 64, 64, 64, g.da1, 64, s.o, pb + E_NN1W);
  for (int e = tid; e < T * 64; e += 256) {   // dO[t][k] = sum_n da1[t][n] Wnn1[n][k]
    const int k = e & 63, t = e >> 6;
    float acc = 0.f;
    for (int n = 0; n < 64; ++n) acc += g.da1[t * 64 + n] * W[E_NN1W + n * 64 + k];
    g.dO[e] = acc;
  }
  __syncthreads();
  for (int e = tid; e < E_HEADS * T * T; e += 256) {   // datt[h][i][j] = sum_d dO[i][h*8+d] v[j][h*8+d]
    const int j = e % T, i = (e / T) % T, h = e / (T * T);
    float acc = 0.f;
#pragma unroll
    for (int d = 0; d < E_HD; ++d) acc += g.dO[i * 64 + h * E_HD + d] * s.qkv[j * 192 + 128 + h * E_HD + d];
    g.datt[(h * HCT_TMAX + i) * HCT_TMAX + j] = acc;
  }
  __syncthreads();
  if (tid < E_HEADS * T) {   // the softmax's backward, with the score scale folded in
    const int i = tid % T, h = tid / T;
    const float* a = s.att + (h * HCT_TMAX + i) * HCT_TMAX;
    float* da = g.datt + (h * HCT_TMAX + i) * HCT_TMAX;
    float r = 0.f;
    for (int j = 0; j < T; ++j) r += a[j] * da[j];
    for (int j = 0; j < T; ++j) da[j] = a[j] * (da[j] - r) * 0.125f;
  }
  __syncthreads();
  for (int e = tid; e < T * 192; e += 256) {
    const int c = e % 192, t = e / 192;
    const int which = c >> 6, hd = c & 63, h = hd >> 3;
    float acc = 0.f;
    if (which == 0) {
      for (int j = 0; j < T; ++j) acc += g.datt[(h * HCT_TMAX + t) * HCT_TMAX + j] * s.qkv[j * 192 + 64 + hd];
    } else if (which == 1) {
      for (int i = 0; i < T; ++i) acc += g.datt[(h * HCT_TMAX + i) * HCT_TMAX + t] * s.qkv[i * 192 + hd];
    } else {
      for (int i = 0; i < T; ++i) acc += s.att[(h * HCT_TMAX + i) * HCT_TMAX + t] * g.dO[i * 64 + hd];
    }
    g.dqkv[e] = acc;
  }
  __syncthreads();
  hct_colsum(T, 192, 192, g.dqkv, pb + E_QKVB);
  hct_outer(T, 192, 64, 192, g.dqkv, 64, s.xn, pb + E_QKVW);
  for (int e = tid; e < T * 64; e += 256) {   // dxn[t][k] = sum_c dqkv[t][c] Wqkv[c][k]
    const int k = e & 63, t = e >> 6;
    float acc = 0.f;
    for (int c = 0; c < 192; ++c) acc += g.dqkv[t * 192 + c] * W[E_QKVW + c * 64 + k];
    g.dxn[e] = acc;
  }
  __syncthreads();
  hct_ln_wgrad(T, s.x, g.dxn, s.mu1, s.rs1, pb + E_LN1W, pb + E_LN1B);
  hct_ln_rows_bwd(T, s.x, g.dxn, W + E_LN1W, s.mu1, s.rs1, g.dx2, true);
  __syncthreads();
  float* dXb = dX + br * strideDX + (long)b * T * 64;
  for (int e = tid; e < T * 64; e += 256) dXb[e] = g.dx2[e];
}

static inline bool hct_p_ok(float p) { return p >= 0.f && p < 1.f; }

static inline bool hct_seq_ok(int B, int T, long stride) {
  return B > 0 && B <= 65535 && T >= 2 && T <= HCT_TMAX && stride >= (long)B * T * HCT_F &&
         2L * B * T * E_MASK < (1L << 31);
}

static int hct_encoder_fwd_launch(int B, int T, const float* X, long strideX, const float* W0, const float* W1,
                                  float pa0, float ph0, float po0, float pa1, float ph1, float po1,
                                  unsigned long long seed, const unsigned long long* seed_dev, float* Y, long strideY,
                                  unsigned char* mask, hipStream_t stream) {
  VC_REQUIRE(hct_seq_ok(B, T, strideX) && strideY >= (long)B * T * HCT_F);
  VC_REQUIRE(hct_p_ok(pa0) && hct_p_ok(ph0) && hct_p_ok(po0) && hct_p_ok(pa1) && hct_p_ok(ph1) && hct_p_ok(po1));
  const bool any = pa0 > 0.f || ph0 > 0.f || po0 > 0.f || pa1 > 0.f || ph1 > 0.f || po1 > 0.f;
  VC_REQUIRE(X && W0 && W1 && Y && (mask || !any));
  VC_REQUIRE((((uintptr_t)W0 | (uintptr_t)W1) & 15) == 0);
  const EncP p0{pa0, ph0, po0}, p1{pa1, ph1, po1};
  hipLaunchKernelGGL(hct_encoder_fwd, dim3(B, 2), dim3(256), 0, stream, B, T, X, strideX, W0, W1, p0, p1, seed,
                     seed_dev, Y, strideY, mask);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

VC_API int vc_hct_encoder_fwd(int B, int T, const float* X, long strideX, const float* W0, const float* W1, float pa0,
                              float ph0, float po0, float pa1, float ph1, float po1, unsigned long long seed, float* Y,
                              long strideY, unsigned char* mask, hipStream_t stream) {
  return hct_encoder_fwd_launch(B, T, X, strideX, W0, W1, pa0, ph0, po0, pa1, ph1, po1, seed, nullptr, Y, strideY, mask,
                                stream);
}

VC_API int vc_hct_encoder_fwd_ds(int B, int T, const float* X, long strideX, const float* W0, const float* W1,
                                 float pa0, float ph0, float po0, float pa1, float ph1, float po1,
                                 const unsigned long long* seed_dev, unsigned long long site_offset, float* Y,
                                 long strideY, unsigned char* mask, hipStream_t stream) {
  VC_REQUIRE(seed_dev);
  return hct_encoder_fwd_launch(B, T, X, strideX, W0, W1, pa0, ph0, po0, pa1, ph1, po1, site_offset, seed_dev, Y,
                                strideY, mask, stream);
}

VC_API int vc_hct_encoder_bwd(int B, int T, const float* X, long strideX, const float* W0, const float* W1, float pa0,
                              float ph0, float po0, float pa1, float ph1, float po1, const unsigned char* mask,
                              const float* dY, long strideDY, float* dX, long strideDX, float* dW0, float* dW1,
                              float* ws, long ws_floats, hipStream_t stream) {
  VC_REQUIRE(hct_seq_ok(B, T, strideX) && strideDY >= (long)B * T * HCT_F && strideDX >= (long)B * T * HCT_F);
  VC_REQUIRE(hct_p_ok(pa0) && hct_p_ok(ph0) && hct_p_ok(po0) && hct_p_ok(pa1) && hct_p_ok(ph1) && hct_p_ok(po1));
  const bool any = pa0 > 0.f || ph0 > 0.f || po0 > 0.f || pa1 > 0.f || ph1 > 0.f || po1 > 0.f;
  VC_REQUIRE(X && W0 && W1 && dY && dX && dW0 && dW1 && (mask || !any));
  VC_REQUIRE((((uintptr_t)W0 | (uintptr_t)W1) & 15) == 0);
  VC_REQUIRE(ws && 2L * B * E_SIZE <= ws_floats);
  const EncP p0{pa0, ph0, po0}, p1{pa1, ph1, po1};
  hipLaunchKernelGGL(hct_encoder_bwd, dim3(B, 2), dim3(256), 0, stream, B, T, X, strideX, W0, W1, p0, p1, mask, dY,
                     strideDY, dX, strideDX, ws);
  VC_CHECK_LAUNCH();
  int rc = launch_sum_rows(B, E_SIZE, ws, E_SIZE, 0, dW0, 0.f, stream);
  if (rc) return rc;
  return launch_sum_rows(B, E_SIZE, ws + (long)B * E_SIZE, E_SIZE, 0, dW1, 0.f, stream);
}

// ---------------------------------------------------------------- cross-token attention
// the packed weights of one direction (LayerNormalize(64, CTAttention(64, heads 8, dim_head 64))), parameter order
#define C_LNW 0
#define C_LNB 64
#define C_WQ 128          // to_q  [512][64]
#define C_WK 32896        // to_kv [1024][64]: rows 0..511 the keys, 512..1023 the values
#define C_WV 65664
#define C_WO 98432        // to_out [64][512]
#define C_BO 131200
#define C_SIZE VC_HCT_CT_FLOATS
#define C_HEADS 8
#define C_SCALE 0.125f    // dim_head^-0.5 = 64^-0.5

// The query is one row, so per head h the keys and values never have to be formed:
//   score[h][j] = q_h . (Wk_h c_j) = (Wk_h^T q_h) . c_j = r_h . c_j,   sum_j a[h][j] (Wv_h c_j) = Wv_h (sum_j a[h][j] c_j)
// which reads every weight once per sample instead of once per context row.
struct CtFwd {
  float cls[64], c[HCT_TMAX * 64], q[512], r[C_HEADS * 64], a[C_HEADS * HCT_TMAX], ad[C_HEADS * HCT_TMAX];
  float cbar[C_HEADS * 64], o[512], mu, rs;
};

// y[m] = sum_i W[m][i] v[i] for m = tid, tid + 256 (W [512][64] rows, v in LDS)
__device__ __forceinline__ void hct_mv512(const float* __restrict__ W, const float* v, float* y, bool per_head) {
  for (int m = threadIdx.x; m < 512; m += 256) {
    const float4* wr = reinterpret_cast<const float4*>(W + (long)m * 64);
    const float* vp = per_head ? v + (m >> 6) * 64 : v;
    float acc = 0.f;
    for (int k4 = 0; k4 < 16; ++k4) {
      const float4 w = wr[k4];
      acc += vp[k4 * 4] * w.x + vp[k4 * 4 + 1] * w.y + vp[k4 * 4 + 2] * w.z + vp[k4 * 4 + 3] * w.w;
    }
    y[m] = acc;
  }
}

// y[h][i] = sum_d W[h*64+d][i] v[h*64+d] for (h, i) = tid, tid + 256: the per-head transposed product
__device__ __forceinline__ void hct_mtv512(const float* __restrict__ W, const float* v, float* y) {
  for (int e = threadIdx.x; e < 512; e += 256) {
    const int h = e >> 6, i = e & 63;
    float acc = 0.f;
    for (int d = 0; d < 64; ++d) acc += W[(long)(h * 64 + d) * 64 + i] * v[h * 64 + d];
    y[e] = acc;
  }
}

__device__ __forceinline__ void hct_ct_core(CtFwd& s, int T, const float* __restrict__ Xq, const float* __restrict__ Xc,
                                            const float* __restrict__ W, const HctDrop& dp, const HctDrop& dout,
                                            float* __restrict__ out) {
  const int tid = threadIdx.x;
  if (tid < 64) s.cls[tid] = Xq[tid];
  for (int e = 64 + tid; e < T * 64; e += 256) s.c[e] = Xc[e];   // rows 1..T-1: the other branch's patch tokens
  __syncthreads();
  if (tid < 64) {   // wave 0: LayerNorm of the cls row -> context row 0
    const float v = s.cls[tid];
    const float mean = wave_sum(v) * (1.f / 64.f);
    const float d = v - mean;
    const float var = wave_sum(d * d) * (1.f / 64.f);
    const float r = 1.f / sqrtf(var + HCT_LN_EPS);
    s.c[tid] = d * r * W[C_LNW + tid] + W[C_LNB + tid];
    if (tid == 0) {
      s.mu = mean;
      s.rs = r;
    }
  }
  __syncthreads();
  hct_mv512(W + C_WQ, s.c, s.q, false);
  __syncthreads();
  hct_mtv512(W + C_WK, s.q, s.r);
  __syncthreads();
  if (tid < C_HEADS * T) {
    const int j = tid % T, h = tid / T;
    float acc = 0.f;
    for (int i = 0; i < 64; ++i) acc += s.r[h * 64 + i] * s.c[j * 64 + i];
    s.a[h * HCT_TMAX + j] = acc * C_SCALE;
  }
  __syncthreads();
  if (tid < C_HEADS) {
    float* a = s.a + tid * HCT_TMAX;
    float m = -INFINITY, z = 0.f;
    for (int j = 0; j < T; ++j) m = fmaxf(m, a[j]);
    for (int j = 0; j < T; ++j) {
      a[j] = __expf(a[j] - m);
      z += a[j];
    }
    const float inv = 1.f / z;
    for (int j = 0; j < T; ++j) {
      a[j] *= inv;
      s.ad[tid * HCT_TMAX + j] = dp.apply(tid * T + j, a[j]);
    }
  }
  __syncthreads();
  for (int e = tid; e < 512; e += 256) {
    const int h = e >> 6, i = e & 63;
    float acc = 0.f;
    for (int j = 0; j < T; ++j) acc += s.ad[h * HCT_TMAX + j] * s.c[j * 64 + i];
    s.cbar[e] = acc;
  }
  __syncthreads();
  hct_mv512(W + C_WV, s.cbar, s.o, true);
  __syncthreads();
  if (out) {   // y[e] = bo[e] + Wo[e] . o: four lanes per output, combined in a fixed order
    const int e = tid >> 2, part = tid & 3;
    const float4* wr = reinterpret_cast<const float4*>(W + C_WO + (long)e * 512 + part * 128);
    const float* op = s.o + part * 128;
    float acc = 0.f;
    for (int k4 = 0; k4 < 32; ++k4) {
      const float4 w = wr[k4];
      acc += op[k4 * 4] * w.x + op[k4 * 4 + 1] * w.y + op[k4 * 4 + 2] * w.z + op[k4 * 4 + 3] * w.w;
    }
    acc += __shfl_xor(acc, 1, 64);
    acc += __shfl_xor(acc, 2, 64);
    if (part == 0) out[e] = s.cls[e] + dout.apply(e, acc + W[C_BO + e]);
  }
}

struct CtP {
  float pp, po;
};

// block (b, d): direction d's query is branch d's cls row, its context branch 1 - d's patch rows
static __global__ __launch_bounds__(256) void hct_ctattn_fwd(int B, int T, const float* __restrict__ X, long strideX,
                                                             const float* __restrict__ W0, const float* __restrict__ W1,
                                                             CtP p0, CtP p1, unsigned long long seed,
                                                             const unsigned long long* __restrict__ seed_dev,
                                                             float* __restrict__ out, unsigned char* __restrict__ mask) {
  __shared__ CtFwd s;
  seed = vc_site_seed(seed, seed_dev);
  const int b = blockIdx.x, d = blockIdx.y;
  const CtP p = d ? p1 : p0;
  const long mb = ((long)d * B + b) * (C_HEADS * T + 64);
  const HctDrop dp = hct_drop(mask, mb, p.pp, seed, true);
  const HctDrop dout = hct_drop(mask, mb + C_HEADS * T, p.po, seed, true);
  hct_ct_core(s, T, X + d * strideX + (long)b * T * 64, X + (1 - d) * strideX + (long)b * T * 64, d ? W1 : W0, dp, dout,
              out + ((long)d * B + b) * 64);
}

struct CtBwd {
  float dy[64], dO[512], dcbar[C_HEADS * 64], ds[C_HEADS * HCT_TMAX], dr[C_HEADS * 64], dq[512], dc[HCT_TMAX * 64];
  float red[4 * 64];
};

static __global__ __launch_bounds__(256) void hct_ctattn_bwd(int B, int T, const float* __restrict__ X, long strideX,
                                                             const float* __restrict__ W0, const float* __restrict__ W1,
                                                             CtP p0, CtP p1, const unsigned char* __restrict__ mask,
                                                             const float* __restrict__ dout_g, float* __restrict__ dX,
                                                             long strideDX, float* __restrict__ part) {
  __shared__ CtFwd s;
  __shared__ CtBwd g;
  const int b = blockIdx.x, d = blockIdx.y, tid = threadIdx.x;
  const CtP p = d ? p1 : p0;
  const float* W = d ? W1 : W0;
  const long mb = ((long)d * B + b) * (C_HEADS * T + 64);
  unsigned char* mk = const_cast<unsigned char*>(mask);
  const HctDrop dp = hct_drop(mk, mb, p.pp, 0, false);
  const HctDrop dou = hct_drop(mk, mb + C_HEADS * T, p.po, 0, false);
  hct_ct_core(s, T, X + d * strideX + (long)b * T * 64, X + (1 - d) * strideX + (long)b * T * 64, W, dp, dou, nullptr);
  float* pb = part + ((long)d * B + b) * C_SIZE;
  const float* dob = dout_g + ((long)d * B + b) * 64;
  if (tid < 64) {
    const float v = dou.apply(tid, dob[tid]);
    g.dy[tid] = v;
    pb[C_BO + tid] = v;
  }
  __syncthreads();
  for (int e = tid; e < 64 * 512; e += 256) pb[C_WO + e] = g.dy[e >> 9] * s.o[e & 511];
  for (int m = tid; m < 512; m += 256) {   // dO[m] = sum_e Wo[e][m] dy[e]
    float acc = 0.f;
    for (int e = 0; e < 64; ++e) acc += W[C_WO + (long)e * 512 + m] * g.dy[e];
    g.dO[m] = acc;
  }
  __syncthreads();
  for (int e = tid; e < 512 * 64; e += 256) pb[C_WV + e] = g.dO[e >> 6] * s.cbar[(e >> 12) * 64 + (e & 63)];
  hct_mtv512(W + C_WV, g.dO, g.dcbar);
  __syncthreads();
  if (tid < C_HEADS * T) {   // d(dropped probability)[h][j] = dcbar[h] . c[j], then the probability dropout
    const int j = tid % T, h = tid / T;
    float acc = 0.f;
    for (int i = 0; i < 64; ++i) acc += g.dcbar[h * 64 + i] * s.c[j * 64 + i];
    g.ds[h * HCT_TMAX + j] = dp.apply(h * T + j, acc);
  }
  __syncthreads();
  if (tid < C_HEADS) {
    const float* a = s.a + tid * HCT_TMAX;
    float* da = g.ds + tid * HCT_TMAX;
    float r = 0.f;
    for (int j = 0; j < T; ++j) r += a[j] * da[j];
    for (int j = 0; j < T; ++j) da[j] = a[j] * (da[j] - r) * C_SCALE;
  }
  __syncthreads();
  for (int e = tid; e < 512; e += 256) {   // dr[h][i] = sum_j ds[h][j] c[j][i]
    const int h = e >> 6, i = e & 63;
    float acc = 0.f;
    for (int j = 0; j < T; ++j) acc += g.ds[h * HCT_TMAX + j] * s.c[j * 64 + i];
    g.dr[e] = acc;
  }
  for (int e = tid; e < T * 64; e += 256) {   // dc[j][i] = sum_h ad[h][j] dcbar[h][i] + ds[h][j] r[h][i]
    const int j = e >> 6, i = e & 63;
    float acc = 0.f;
#pragma unroll
    for (int h = 0; h < C_HEADS; ++h)
      acc += s.ad[h * HCT_TMAX + j] * g.dcbar[h * 64 + i] + g.ds[h * HCT_TMAX + j] * s.r[h * 64 + i];
    g.dc[e] = acc;
  }
  __syncthreads();
  for (int e = tid; e < 512 * 64; e += 256) pb[C_WK + e] = s.q[e >> 6] * g.dr[(e >> 12) * 64 + (e & 63)];
  hct_mv512(W + C_WK, g.dr, g.dq, true);
  __syncthreads();
  for (int e = tid; e < 512 * 64; e += 256) pb[C_WQ + e] = g.dq[e >> 6] * s.c[e & 63];
  {   // dn[i] = sum_m Wq[m][i] dq[m] + dc[0][i]: four 128-row slices, combined in a fixed order
    const int i = tid & 63, sl = tid >> 6;
    float acc = 0.f;
    for (int m = sl * 128; m < sl * 128 + 128; ++m) acc += W[C_WQ + (long)m * 64 + i] * g.dq[m];
    g.red[sl * 64 + i] = acc;
  }
  __syncthreads();
  float* dXq = dX + d * strideDX + (long)b * T * 64;
  float* dXc = dX + (1 - d) * strideDX + (long)b * T * 64;
  if (tid < 64) {   // wave 0: the LayerNorm's backward and the residual
    const float dn = ((g.red[tid] + g.red[64 + tid]) + (g.red[128 + tid] + g.red[192 + tid])) + g.dc[tid];
    const float xh = (s.cls[tid] - s.mu) * s.rs;
    pb[C_LNW + tid] = dn * xh;
    pb[C_LNB + tid] = dn;
    const float gx = dn * W[C_LNW + tid];
    const float m1 = wave_sum(gx) * (1.f / 64.f);
    const float m2 = wave_sum(gx * xh) * (1.f / 64.f);
    dXq[tid] = dob[tid] + s.rs * (gx - m1 - xh * m2);
  }
  for (int e = 64 + tid; e < T * 64; e += 256) dXc[e] = g.dc[e];
}

static int hct_ctattn_fwd_launch(int B, int T, const float* X, long strideX, const float* W0, const float* W1,
                                 float pp0, float po0, float pp1, float po1, unsigned long long seed,
                                 const unsigned long long* seed_dev, float* out, unsigned char* mask,
                                 hipStream_t stream) {
  VC_REQUIRE(hct_seq_ok(B, T, strideX));
  VC_REQUIRE(hct_p_ok(pp0) && hct_p_ok(po0) && hct_p_ok(pp1) && hct_p_ok(po1));
  const bool any = pp0 > 0.f || po0 > 0.f || pp1 > 0.f || po1 > 0.f;
  VC_REQUIRE(X && W0 && W1 && out && (mask || !any));
  VC_REQUIRE((((uintptr_t)W0 | (uintptr_t)W1) & 15) == 0);
  const CtP p0{pp0, po0}, p1{pp1, po1};
  hipLaunchKernelGGL(hct_ctattn_fwd, dim3(B, 2), dim3(256), 0, stream, B, T, X, strideX, W0, W1, p0, p1, seed,
                     seed_dev, out, mask);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

VC_API int vc_hct_ctattn_fwd(int B, int T, const float* X, long strideX, const float* W0, const float* W1, float pp0,
                             float po0, float pp1, float po1, unsigned long long seed, float* out, unsigned char* mask,
                             hipStream_t stream) {
  return hct_ctattn_fwd_launch(B, T, X, strideX, W0, W1, pp0, po0, pp1, po1, seed, nullptr, out, mask, stream);
}

VC_API int vc_hct_ctattn_fwd_ds(int B, int T, const float* X, long strideX, const float* W0, const float* W1,
                                float pp0, float po0, float pp1, float po1, const unsigned long long* seed_dev,
                                unsigned long long site_offset, float* out, unsigned char* mask, hipStream_t stream) {
  VC_REQUIRE(seed_dev);
  return hct_ctattn_fwd_launch(B, T, X, strideX, W0, W1, pp0, po0, pp1, po1, site_offset, seed_dev, out, mask, stream);
}

VC_API int vc_hct_ctattn_bwd(int B, int T, const float* X, long strideX, const float* W0, const float* W1, float pp0,
                             float po0, float pp1, float po1, const unsigned char* mask, const float* dout, float* dX,
                             long strideDX, float* dW0, float* dW1, float* ws, long ws_floats, hipStream_t stream) {
  VC_REQUIRE(hct_seq_ok(B, T, strideX) && strideDX >= (long)B * T * HCT_F);
  VC_REQUIRE(hct_p_ok(pp0) && hct_p_ok(po0) && hct_p_ok(pp1) && hct_p_ok(po1));
  const bool any = pp0 > 0.f || po0 > 0.f || pp1 > 0.f || po1 > 0.f;
  VC_REQUIRE(X && W0 && W1 && dout && dX && dW0 && dW1 && (mask || !any));
  VC_REQUIRE((((uintptr_t)W0 | (uintptr_t)W1) & 15) == 0);
  VC_REQUIRE(ws && 2L * B * C_SIZE <= ws_floats);
  const CtP p0{pp0, po0}, p1{pp1, po1};
  hipLaunchKernelGGL(hct_ctattn_bwd, dim3(B, 2), dim3(256), 0, stream, B, T, X, strideX, W0, W1, p0, p1, mask, dout, dX,
                     strideDX, ws);
  VC_CHECK_LAUNCH();
  int rc = launch_sum_rows(B, C_SIZE, ws, C_SIZE, 0, dW0, 0.f, stream);
  if (rc) return rc;
  return launch_sum_rows(B, C_SIZE, ws + (long)B * C_SIZE, C_SIZE, 0, dW1, 0.f, stream);
}

// Single-head non-local cross attention of GLfusionBlock (NONLocalBlock2D, sub_sample=True;
// Mutimodality_Mamba7.py:140-159): f = theta(x)^T phi(y) WITHOUT 1/sqrt(d) scaling,
// softmax over the max-pooled keys, o = f g(z).  Per batch element the problem is tiny
// (queries S = 49 / 25, keys P = 9 / 4, inter channels Ci = 128 / 72): keys and values live in
// LDS, one wave per query row, wave64 shuffle reductions for the dot products and the softmax.
// Forward: a workgroup of 16 waves owns 16 query rows of one batch element (grid B x S/16).
// Backward: a 16-wave workgroup owns a whole batch element, since d(phi|g) reduces over all
// of its query rows in LDS (fixed order, no atomics).
//
// Layouts: theta [B*S, Ci]; pooled phi|g [B*P, 2*Ci] (phi in columns [0,Ci), g in [Ci,2Ci));
// att (saved softmax) [B, S, P]; o [B*S, Ci].
#include "common.h"

namespace {

constexpr int MAXP = 16;  // 2x2-pooled 9x9 grid (the largest patch the build supports: 11x11 inputs)
constexpr int MAXCI = 256;

// PT = number of pooled keys (compile-time so the per-row score array stays in registers)
constexpr int NT = 1024, NW = NT / 64;

// POOL: the 2x2 max pool of the phi | g map (Mutimodality_Mamba7.py:94) done while staging the keys --
// pg [B][Hs][Hs] rows of 2 Ci (stride ldpg), the window max and its tap as vc_maxpool2_fwd takes them
// (first max in scan order, NaN propagates); the y = 0 workgroup of each batch element stores pooled +
// tap for the backward.  One launch instead of two on the GLfusion forward chain.
template <int PT, bool POOL>
__global__ __launch_bounds__(NT) void nl_fwd(int S, int Ci, const float* __restrict__ theta,
                                             const float* __restrict__ pooled, float* __restrict__ att,
                                             float* __restrict__ o, int Hs, const float* __restrict__ pg, long ldpg,
                                             float* __restrict__ pooled_out, unsigned char* __restrict__ tap_out) {
  constexpr int P = PT;
  extern __shared__ float kv[];  // [P][2*Ci]
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (POOL) {
    const int C2 = 2 * Ci, PWd = Hs >> 1;
    const bool store = blockIdx.y == 0;
    for (int i = threadIdx.x; i < P * C2; i += NT) {
      const int key = i / C2, ch = i - key * C2, ph = key / PWd, pw = key - ph * PWd;
      const float* xb = pg + ((long)(b * Hs + 2 * ph) * Hs + 2 * pw) * ldpg + ch;
      float best = xb[0];
      int bi = 0;
#pragma unroll
      for (int t = 1; t < 4; ++t) {
        const float v = xb[((t >> 1) * Hs + (t & 1)) * ldpg];
        if (v > best || isnan(v)) {
          best = v;
          bi = t;
        }
      }
      kv[i] = best;
      if (store) {
        pooled_out[(long)b * P * C2 + i] = best;
        tap_out[(long)b * P * C2 + i] = (unsigned char)bi;
      }
    }
  } else {
    const float* src = pooled + (long)b * P * 2 * Ci;
    for (int i = threadIdx.x; i < P * 2 * Ci; i += NT) kv[i] = src[i];
  }
  __syncthreads();
  {
    const int s = blockIdx.y * NW + wave;
    if (s >= S) return;
    const float* q = theta + ((long)b * S + s) * Ci;
    float sc[PT];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < P; ++j) {
      float acc = 0.f;
      for (int c = lane; c < Ci; c += 64) acc += q[c] * kv[j * 2 * Ci + c];
      sc[j] = wave_sum(acc);
      mx = fmaxf(mx, sc[j]);
    }
    float den = 0.f;
#pragma unroll
    for (int j = 0; j < P; ++j) {
      sc[j] = __expf(sc[j] - mx);
      den += sc[j];
    }
    const float inv = 1.f / den;
#pragma unroll
    for (int j = 0; j < P; ++j) sc[j] *= inv;
    if (lane < P) {
      float v = 0.f;
#pragma unroll
      for (int j = 0; j < P; ++j)
        if (j == lane) v = sc[j];
      att[((long)b * S + s) * P + lane] = v;
    }
    float* orow = o + ((long)b * S + s) * Ci;
    for (int c = lane; c < Ci; c += 64) {
      float acc = 0.f;
#pragma unroll
      for (int j = 0; j < P; ++j) acc += sc[j] * kv[j * 2 * Ci + Ci + c];
      orow[c] = acc;
    }
  }
}

template <int PT>
__global__ __launch_bounds__(NT) void nl_bwd(int S, int Ci, const float* __restrict__ theta,
                                              const float* __restrict__ pooled, const float* __restrict__ att,
                                              const float* __restrict__ dout, float* __restrict__ dtheta,
                                              float* __restrict__ dpooled) {
  constexpr int P = PT;
  extern __shared__ float sm[];
  float* kv = sm;                   // [P][2Ci]
  float* ds = kv + P * 2 * Ci;      // [S][P] dscore
  float* at = ds + S * P;           // [S][P] att
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* src = pooled + (long)b * P * 2 * Ci;
  for (int i = threadIdx.x; i < P * 2 * Ci; i += NT) kv[i] = src[i];
  for (int i = threadIdx.x; i < S * P; i += NT) at[i] = att[(long)b * S * P + i];
  __syncthreads();
  for (int s = wave; s < S; s += NW) {
    const float* dr = dout + ((long)b * S + s) * Ci;
    float da[PT];
    float dot = 0.f;
#pragma unroll
    for (int j = 0; j < P; ++j) {
      float acc = 0.f;
      for (int c = lane; c < Ci; c += 64) acc += dr[c] * kv[j * 2 * Ci + Ci + c];
      da[j] = wave_sum(acc);
      dot += at[s * P + j] * da[j];
    }
#pragma unroll
    for (int j = 0; j < P; ++j) da[j] = at[s * P + j] * (da[j] - dot);
    if (lane < P) {
      float v = 0.f;
#pragma unroll
      for (int j = 0; j < P; ++j)
        if (j == lane) v = da[j];
      ds[s * P + lane] = v;
    }
    float* dq = dtheta + ((long)b * S + s) * Ci;
    for (int c = lane; c < Ci; c += 64) {
      float acc = 0.f;
#pragma unroll
      for (int j = 0; j < P; ++j) acc += da[j] * kv[j * 2 * Ci + c];
      dq[c] = acc;
    }
  }
  __syncthreads();
  float* dp = dpooled + (long)b * P * 2 * Ci;
  for (int i = threadIdx.x; i < P * 2 * Ci; i += NT) {
    const int j = i / (2 * Ci), c = i - j * (2 * Ci);
    float acc = 0.f;
    if (c < Ci) {
      for (int s = 0; s < S; ++s) acc += ds[s * P + j] * theta[((long)b * S + s) * Ci + c];
    } else {
      for (int s = 0; s < S; ++s) acc += at[s * P + j] * dout[((long)b * S + s) * Ci + c - Ci];
    }
    dp[i] = acc;
  }
}


// ---------------------------------------------------------------- MFMA form (v_mfma_f32_16x16x4_f32)
// The same attention with the key dimension as one 16-wide MFMA tile (P <= 16) and the channels as the
// reduction, in the transposed orientation of the S2EFT attention kernels: a wave owns 16 queries of
// one batch element and computes S^T = phi theta^T (lane (g, c) holds the scores of query c for keys
// 4g..4g+3, so the softmax is 4 in-lane terms plus a cross-row max / sum), then O^T = g^T P^T with
// P^T taken straight from the accumulator (the k order of each MFMA pairs key 4g + s on both
// operands).  The channel reduction of a 16-channel chunk is 4 MFMAs over float4 operand loads: step
// s of lane group g pairs channel 16 kc + 4g + s on both operands.  No LDS: the pooled keys / values
// of an element (<= 16 rows) come from L1 / L2.  Requires Ci % 4 == 0 (float4 rows).
__device__ __forceinline__ f32x4 mfma_x4(f32x4 a, f32x4 b, f32x4 c) {
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, c, 0, 0, 0);
  return c;
}
// float4 of row `row` (stride ld) at channel ch, zero when the row or the channel chunk is out of range
__device__ __forceinline__ f32x4 ld4_or0(const float* base, long ld, bool row_ok, int ch, int Ci) {
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  return (row_ok && ch < Ci) ? *reinterpret_cast<const f32x4*>(base + ch) : z;
}
// cross-row max / sum over the 4 lane groups (lanes c, c+16, c+32, c+48)
__device__ __forceinline__ float xrow_max(float v) {
  return cross_row_max(v);
}

constexpr int NLW = 4;   // waves (16-query tiles) per forward block
constexpr int NACC = 8;  // accumulators of the channel reductions
constexpr int NL_MFMA_FWD_MIN_B = 256;

template <int N>
__device__ __forceinline__ f32x4 tree_sum(const f32x4 (&a)[N]) {
  if constexpr (N == 1) {
    return a[0];
  } else {
    f32x4 h[N / 2];
#pragma unroll
    for (int j = 0; j < N / 2; ++j) h[j] = a[2 * j] + a[2 * j + 1];
    return tree_sum(h);
  }
}

__global__ __launch_bounds__(NLW * 64) void nl_fwd_mfma(int B, int S, int P, int Ci, const float* __restrict__ theta,
                                                        const float* __restrict__ pooled, float* __restrict__ att,
                                                        float* __restrict__ o) {
  const int nqt = (S + 15) >> 4;
  const int unit = blockIdx.x * NLW + (threadIdx.x >> 6);
  if (unit >= B * nqt) return;   // whole wave idle (no barrier in this kernel)
  const int b = unit / nqt, qt = unit - b * nqt;
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const int q = qt * 16 + c;
  const bool q_ok = q < S, k_ok = c < P;
  const long ldp = 2L * Ci;
  const float* th_row = theta + ((long)b * S + (q_ok ? q : 0)) * Ci;
  const float* ph_row = pooled + ((long)b * P + (k_ok ? c : 0)) * ldp;
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  // S^T[key = 4g + r][query = c]; the channel reduction is spread over NACC accumulators (chunk j into
  // accumulator j % NACC) and summed pairwise, so each score is a depth-(4 Ci/(16 NACC) + 3) sum instead
  // of one 4 Ci/16-step chain: the softmax backward cancels (dA - rowsum), and the scores' rounding
  // must stay at the level of a pairwise dot product
  f32x4 acc[NACC];
#pragma unroll
  for (int j = 0; j < NACC; ++j) acc[j] = z;
  for (int kc0 = 0; kc0 < Ci; kc0 += 16 * NACC) {
#pragma unroll
    for (int j = 0; j < NACC; ++j) {
      const int ch = kc0 + 16 * j + 4 * g;
      if (kc0 + 16 * j < Ci)
        acc[j] = mfma_x4(ld4_or0(ph_row, ldp, k_ok, ch, Ci), ld4_or0(th_row, Ci, q_ok, ch, Ci), acc[j]);
    }
  }
  const f32x4 st = tree_sum(acc);
  float sv[4], mx = -INFINITY;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    sv[r] = (4 * g + r < P) ? st[r] : -INFINITY;
    mx = fmaxf(mx, sv[r]);
  }
  mx = xrow_max(mx);
  float den = 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    sv[r] = (4 * g + r < P) ? __expf(sv[r] - mx) : 0.f;
    den += sv[r];
  }
  den = cross_row_sum(den);
  const float inv = 1.f / den;
#pragma unroll
  for (int r = 0; r < 4; ++r) sv[r] *= inv;
  if (q_ok) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (4 * g + r < P) att[((long)b * S + q) * P + 4 * g + r] = sv[r];
  }
  // O^T[d][q] = sum_key G[key][d] P^T[key][q]; A: G[key = 4g + s][d = dc + c], B: register s
  const float* gbase = pooled + (long)b * P * ldp + Ci;
  float* orow = o + ((long)b * S + q) * Ci;
  for (int dc = 0; dc < Ci; dc += 16) {
    const int d = dc + c;
    f32x4 gv;
#pragma unroll
    for (int s2 = 0; s2 < 4; ++s2) gv[s2] = (4 * g + s2 < P && d < Ci) ? gbase[(4 * g + s2) * ldp + d] : 0.f;
    const f32x4 pv = {sv[0], sv[1], sv[2], sv[3]};
    const f32x4 acc = mfma_x4(gv, pv, z);   // O^T[d = dc + 4g + r][q = c]
    if (q_ok && dc + 4 * g < Ci) *reinterpret_cast<f32x4*>(orow + dc + 4 * g) = acc;
  }
}

// Backward: one block per batch element, one wave per 16-query tile (nqt <= 16 waves).
// Pass 1 (wave = query tile): dA^T = G dO^T (MFMA), dS^T = att^T * (dA^T - rowsum), dtheta^T = phi^T dS^T;
// dS and att go to LDS as [query][16].  Pass 2 (wave = channel chunks dc = 16 w, 16 (w + nqt), ...):
// dphi^T = theta^T dS and dg^T = dO^T att, the query reduction walked in 16-query tiles (fixed order).
// POOL: the gradient of the 2x2 max pool that made `pooled` (Mutimodality_Mamba7.py:94) folded in --
// dpg [B][Hs][Hs][2 Ci] (the phi | g maps before pooling) gets each pooled gradient at its window's
// argmax (arg, vc_maxpool2_fwd's record) and 0 elsewhere, as vc_maxpool2_bwd writes it: one launch
// instead of two on the GLfusion backward chain.
template <bool POOL>
__global__ __launch_bounds__(1024) void nl_bwd_mfma(int S, int P, int Ci, const float* __restrict__ theta,
                                                    const float* __restrict__ pooled, const float* __restrict__ att,
                                                    const float* __restrict__ dout, float* __restrict__ dtheta,
                                                    float* __restrict__ dpooled, int Hs,
                                                    const unsigned char* __restrict__ arg) {
  extern __shared__ f32x4 nl_lds[];
  const int nqt = (S + 15) >> 4;
  float* dsL = reinterpret_cast<float*>(nl_lds);   // [nqt * 16][16]
  float* atL = dsL + nqt * 256;                      // [nqt * 16][16]
  const int b = blockIdx.x, wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const long ldp = 2L * Ci;
  const float* pb = pooled + (long)b * P * ldp;
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  if (wave < nqt) {   // pass 1
    const int q = wave * 16 + c;
    const bool q_ok = q < S, k_ok = c < P;
    const float* do_row = dout + ((long)b * S + (q_ok ? q : 0)) * Ci;
    const float* g_row = pb + (k_ok ? c : 0) * ldp + Ci;
    f32x4 acc[NACC];   // dA^T[key = 4g + r][q = c], channel reduction spread as in the forward
#pragma unroll
    for (int j = 0; j < NACC; ++j) acc[j] = z;
    for (int kc0 = 0; kc0 < Ci; kc0 += 16 * NACC) {
#pragma unroll
      for (int j = 0; j < NACC; ++j) {
        const int ch = kc0 + 16 * j + 4 * g;
        if (kc0 + 16 * j < Ci)
          acc[j] = mfma_x4(ld4_or0(g_row, ldp, k_ok, ch, Ci), ld4_or0(do_row, Ci, q_ok, ch, Ci), acc[j]);
      }
    }
    const f32x4 da = tree_sum(acc);
    f32x4 at;
#pragma unroll
    for (int r = 0; r < 4; ++r) at[r] = (q_ok && 4 * g + r < P) ? att[((long)b * S + q) * P + 4 * g + r] : 0.f;
    float dot = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) dot += at[r] * da[r];
    dot = cross_row_sum(dot);
    f32x4 dsv;
#pragma unroll
    for (int r = 0; r < 4; ++r) dsv[r] = at[r] * (da[r] - dot);
    *reinterpret_cast<f32x4*>(dsL + q * 16 + 4 * g) = dsv;
    *reinterpret_cast<f32x4*>(atL + q * 16 + 4 * g) = at;
    // dtheta^T[d][q] = sum_key phi[key][d] dS^T[key][q]
    float* dq = dtheta + ((long)b * S + q) * Ci;
    for (int dc = 0; dc < Ci; dc += 16) {
      const int d = dc + c;
      f32x4 pv;
#pragma unroll
      for (int s2 = 0; s2 < 4; ++s2) pv[s2] = (4 * g + s2 < P && d < Ci) ? pb[(4 * g + s2) * ldp + d] : 0.f;
      const f32x4 acc = mfma_x4(pv, dsv, z);
      if (q_ok && dc + 4 * g < Ci) *reinterpret_cast<f32x4*>(dq + dc + 4 * g) = acc;
    }
  }
  __syncthreads();
  // pass 2: dphi^T[d][key] = sum_q theta[q][d] dS[q][key], dg^T[d][key] = sum_q dO[q][d] att[q][key]
  const int nw = blockDim.x >> 6;
  const float* thb = theta + (long)b * S * Ci;
  const float* dob = dout + (long)b * S * Ci;
  for (int dc = wave * 16; dc < Ci; dc += nw * 16) {
    const int d = dc + c;
    const bool d_ok = d < Ci;
    f32x4 aphi4[4] = {z, z, z, z}, ag4[4] = {z, z, z, z};   // [d = dc + 4g + r][key = c], tile qt -> qt % 4
    for (int qt = 0; qt < nqt; ++qt) {
      f32x4 tv, ov, sb, ab;
#pragma unroll
      for (int s2 = 0; s2 < 4; ++s2) {
        const int q = qt * 16 + 4 * g + s2;
        const bool ok = q < S && d_ok;
        tv[s2] = ok ? thb[(long)q * Ci + d] : 0.f;
        ov[s2] = ok ? dob[(long)q * Ci + d] : 0.f;
        sb[s2] = dsL[q * 16 + c];   // rows q >= S hold 0 (written by pass 1 from zero att)
        ab[s2] = atL[q * 16 + c];
      }
      aphi4[qt & 3] = mfma_x4(tv, sb, aphi4[qt & 3]);
      ag4[qt & 3] = mfma_x4(ov, ab, ag4[qt & 3]);
    }
    const f32x4 aphi = tree_sum(aphi4), ag = tree_sum(ag4);
    if (c < P && dc + 4 * g < Ci) {
      if (POOL) {
        // key c = pooled pixel (ph, pw) of a (Hs / 2)^2 grid; window pixel (2 ph + (a >> 1), 2 pw + (a & 1))
        const int PW = Hs >> 1, ph = c / PW, pw = c - ph * PW;
        const unsigned char* ab = arg + ((long)b * P + c) * ldp + dc + 4 * g;
        float* db = dpooled + (long)b * Hs * Hs * ldp + dc + 4 * g;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          float* w = db + ((2 * ph + (a >> 1)) * Hs + 2 * pw + (a & 1)) * ldp;
          f32x4 vp, vg;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            vp[r] = ab[r] == a ? aphi[r] : 0.f;
            vg[r] = ab[r + Ci] == a ? ag[r] : 0.f;
          }
          *reinterpret_cast<f32x4*>(w) = vp;
          *reinterpret_cast<f32x4*>(w + Ci) = vg;
        }
      } else {
        float* w = dpooled + ((long)b * P + c) * ldp + dc + 4 * g;
        *reinterpret_cast<f32x4*>(w) = aphi;
        *reinterpret_cast<f32x4*>(w + Ci) = ag;
      }
    }
  }
  if (POOL && (Hs & 1)) {   // the last row and column are in no window: gradient 0
    const int nl = 2 * Hs - 1;   // pixels (Hs - 1, *) and (*, Hs - 1)
    float* db = dpooled + (long)b * Hs * Hs * ldp;
    for (int i = threadIdx.x; i < nl * (int)(ldp / 4); i += blockDim.x) {
      const int px = i / (int)(ldp / 4), c4 = i - px * (int)(ldp / 4);
      const int pix = px < Hs ? (Hs - 1) * Hs + px : (px - Hs) * Hs + Hs - 1;
      *reinterpret_cast<f32x4*>(db + (long)pix * ldp + 4 * c4) = z;
    }
  }
}

}  // namespace

VC_API int vc_maxpool2_bwd(int B, int H, int W, int C, const float* dy, const unsigned char* arg, float* dx, long lddx,
                           hipStream_t stream);

// float4 row accesses of the MFMA forms need 16-B aligned bases (rows are 16-B multiples when Ci % 4 == 0)
static bool aligned16(const void* a, const void* b, const void* c) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}
// knob NL_LEGACY (probe library only; bit 0 forward, bit 1 backward): the wave-per-row kernels even where
// the MFMA form applies
static bool nl_legacy(int bit) { return (vc_knob("VITCNN_NL_LEGACY", 0) >> bit) & 1; }

VC_API int vc_nonlocal_attn_fwd(int B, int S, int P, int Ci, const float* theta, const float* pooled, float* att,
                                float* o, hipStream_t stream) {
  VC_REQUIRE(B > 0 && S > 0 && P > 0 && P <= MAXP && Ci > 0 && Ci <= MAXCI);
  // MFMA form for the large batches of whole-image inference (test(): thousands of windows per call,
  // where the wave-per-row grid is B x S/16 blocks of 1024 threads).  Below NL_MFMA_FWD_MIN_B (the
  // training batches) the wave-per-row forward stays: both are fp32-accurate (the MFMA scores are
  // pairwise-summed), but the reference-golden B = 4 gradient test's ill-conditioned TokenLearner
  // tensors downstream (hsi2 channel tokenizers, BN(1) of a near-constant map) sit within the fp32
  // reference's own error with the wave-per-row rounding and outside it with the MFMA rounding
  // (tools/nl_diag3.py: 0 vs 6 of 671 tensors), and the training forward gains nothing measurable
  // (the non-local branch runs on a side lane).
  const bool legacy_p = P == 4 || P == 9 || P == 16;   // key counts the wave-per-row kernel is built for
  if (Ci % 4 == 0 && (B >= NL_MFMA_FWD_MIN_B || !legacy_p) && aligned16(theta, pooled, o) && !nl_legacy(0)) {
    const long units = (long)B * ((S + 15) / 16);
    VC_REQUIRE_I32(units * 64);
    hipLaunchKernelGGL(nl_fwd_mfma, dim3((unsigned)vc_cdiv(units, NLW)), dim3(NLW * 64), 0, stream, B, S, P, Ci,
                       theta, pooled, att, o);
    VC_CHECK_LAUNCH();
    return VC_OK;
  }
  const size_t sm = sizeof(float) * (size_t)P * 2 * Ci;
#define VC_NL_FWD(PT_)                                                                                       \
  hipLaunchKernelGGL((nl_fwd<PT_, false>), dim3(B, vc_cdiv(S, NW)), dim3(NT), sm, stream, S, Ci, theta, pooled, \
                     att, o, 0, nullptr, 0L, nullptr, nullptr)
  switch (P) {  // pooled key counts of 5x5 / 7x7 / 9x9 query grids; 1: the 3x3 grid where the MFMA form is ruled out
    case 1: VC_NL_FWD(1); break;
    case 4: VC_NL_FWD(4); break;
    case 9: VC_NL_FWD(9); break;
    case 16: VC_NL_FWD(16); break;
    default: return VC_EINVAL;
  }
#undef VC_NL_FWD
  VC_CHECK_LAUNCH();
  return VC_OK;
}

VC_API int vc_maxpool2_fwd(int B, int H, int W, int C, const float* x, long ldx, float* y, unsigned char* arg,
                           hipStream_t stream);

// vc_maxpool2_fwd of the phi | g map + vc_nonlocal_attn_fwd in one launch where the wave-per-row forward
// runs (the training batches); the two launches otherwise
VC_API int vc_nonlocal_attn_pool_fwd(int B, int S, int P, int Ci, int Hs, const float* theta, const float* pg,
                                     long ldpg, float* pooled, unsigned char* arg, float* att, float* o,
                                     hipStream_t stream) {
  VC_REQUIRE(B > 0 && S > 0 && P > 0 && P <= MAXP && Ci > 0 && Ci <= MAXCI && Hs >= 2 && (Hs / 2) * (Hs / 2) == P &&
             ldpg >= 2 * Ci);
  const bool legacy_p = P == 4 || P == 9 || P == 16;
  const bool mfma = Ci % 4 == 0 && (B >= NL_MFMA_FWD_MIN_B || !legacy_p) && aligned16(theta, pooled, o) &&
                    !nl_legacy(0);
  if (mfma || !legacy_p) {
    const int rc = vc_maxpool2_fwd(B, Hs, Hs, 2 * Ci, pg, ldpg, pooled, arg, stream);
    if (rc) return rc;
    return vc_nonlocal_attn_fwd(B, S, P, Ci, theta, pooled, att, o, stream);
  }
  VC_REQUIRE_I32((long)B * Hs * Hs * ldpg);
  const size_t sm = sizeof(float) * (size_t)P * 2 * Ci;
#define VC_NL_PFWD(PT_)                                                                                       \
  hipLaunchKernelGGL((nl_fwd<PT_, true>), dim3(B, vc_cdiv(S, NW)), dim3(NT), sm, stream, S, Ci, theta, nullptr, \
                     att, o, Hs, pg, ldpg, pooled, arg)
  switch (P) {
    case 4: VC_NL_PFWD(4); break;
    case 9: VC_NL_PFWD(9); break;
    default: VC_NL_PFWD(16); break;
  }
#undef VC_NL_PFWD
  VC_CHECK_LAUNCH();
  return VC_OK;
}

VC_API int vc_nonlocal_attn_bwd(int B, int S, int P, int Ci, const float* theta, const float* pooled, const float* att,
                                const float* dout, float* dtheta, float* dpooled, hipStream_t stream) {
  VC_REQUIRE(B > 0 && S > 0 && P > 0 && P <= MAXP && Ci > 0 && Ci <= MAXCI);
  if (Ci % 4 == 0 && S <= 256 && aligned16(theta, pooled, dout) && aligned16(dtheta, dpooled, dpooled) &&
      !nl_legacy(1)) {
    // MFMA form: one wave per 16-query tile (at least 4 for pass 2)
    const int nqt = (S + 15) / 16;
    const int nw = std::max(nqt, 4);
    hipLaunchKernelGGL(nl_bwd_mfma<false>, dim3(B), dim3(nw * 64), sizeof(float) * nqt * 512, stream, S, P, Ci,
                       theta, pooled, att, dout, dtheta, dpooled, 0, nullptr);
    VC_CHECK_LAUNCH();
    return VC_OK;
  }
  const size_t sm = sizeof(float) * ((size_t)P * 2 * Ci + 2 * (size_t)S * P);
  VC_REQUIRE(sm <= 160 * 1024);
#define VC_NL_BWD(PT_) \
  hipLaunchKernelGGL((nl_bwd<PT_>), dim3(B), dim3(NT), sm, stream, S, Ci, theta, pooled, att, dout, dtheta, dpooled)
  switch (P) {
    case 1: VC_NL_BWD(1); break;   // (the 3x3 grid's one pooled key, Ci % 4 != 0)
    case 4: VC_NL_BWD(4); break;
    case 9: VC_NL_BWD(9); break;
    case 16: VC_NL_BWD(16); break;
    default: return VC_EINVAL;
  }
#undef VC_NL_BWD
  VC_CHECK_LAUNCH();
  return VC_OK;
}

// vc_nonlocal_attn_bwd + vc_maxpool2_bwd in one launch where the MFMA form applies (dpg [B][Hs][Hs][2 Ci],
// overwritten; arg: vc_maxpool2_fwd's window argmax); the two launches otherwise
VC_API int vc_nonlocal_attn_pool_bwd(int B, int S, int P, int Ci, int Hs, const float* theta, const float* pooled,
                                     const float* att, const float* dout, const unsigned char* arg, float* dtheta,
                                     float* dpooled, float* dpg, hipStream_t stream) {
  VC_REQUIRE(B > 0 && S > 0 && P > 0 && P <= MAXP && Ci > 0 && Ci <= MAXCI && Hs >= 2 && (Hs / 2) * (Hs / 2) == P);
  if (Ci % 4 == 0 && S <= 256 && aligned16(theta, pooled, dout) && aligned16(dtheta, dpg, dpg) && !nl_legacy(1)) {
    const int nqt = (S + 15) / 16;
    const int nw = std::max(nqt, 4);
    hipLaunchKernelGGL(nl_bwd_mfma<true>, dim3(B), dim3(nw * 64), sizeof(float) * nqt * 512, stream, S, P, Ci, theta,
                       pooled, att, dout, dtheta, dpg, Hs, arg);
    VC_CHECK_LAUNCH();
    return VC_OK;
  }
  const int rc = vc_nonlocal_attn_bwd(B, S, P, Ci, theta, pooled, att, dout, dtheta, dpooled, stream);
  if (rc) return rc;
  return vc_maxpool2_bwd(B, Hs, Hs, 2 * Ci, dpooled, arg, dpg, 2 * Ci, stream);
}

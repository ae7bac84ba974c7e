// MHST's pyramidal grouped "whole-depth" convolutions on 8 x 8 maps as implicit GEMMs on v_mfma_f32_16x16x4_f32
// (A: row = lane & 15, k = lane >> 4; B: col = lane & 15, k = lane >> 4; D: col = lane & 15, row = (lane >> 4) * 4 + r).
// Formulas and the alignment contract: include/vitcnn.h (vc_mhst_pconv_*); the formulation: DESIGN.md section 28.
// Exact fp32: an MFMA is a k-ordered fmaf chain.  No atomics; every partial is summed in a fixed order.
//
// Per group the three directions are skinny GEMMs whose N is padded to 16 with zero weights:
//   fwd    M = (b, position)  N = O/G          K = (tap, depth, channel of the group)
//   dgrad  M = (b, position)  N = (depth, channel of the group) in tiles of 16    K = (tap, output of the group)
//   wgrad  M = O/G            N = (depth, channel of the group) in tiles of 16    K = (b, position), one tile per tap
// The weight is re-laid [k][16] into the workspace by a pack launch per call (fwd, dgrad), so a wave's B operand is one
// 256-byte run.  Only a group's own channels / outputs are ever read: row padding and the neighbours' columns never
// reach an operand, and a lane whose tap falls outside the map feeds 0 without reading.  A (tile, tap) pair with no
// lane inside the map is skipped before it costs an MFMA (wave-uniform ballot).
#include "common.h"

namespace {

struct PShape {
  int B, D, C, O, G, KS, cg, og, lcg, log, KK, ps;
};

__host__ __device__ inline int pc_chunk(int cg) { return cg <= 16 ? VC_MHST_PCONV_CHUNK : VC_MHST_PCONV_CHUNK / 2; }

constexpr int PC_U = 8;   // MFMA steps whose operands are fetched together
constexpr int PC_WLDS_FLOATS = 8192;   // dgrad keeps a group's weight of up to 32 KB in LDS, unpacked
constexpr int PC_XS = 2 * VC_MHST_PCONV_CHUNK * 64 * 17;   // fwd LDS floats: 2 samples x chunk x 64 x (cg + 1)

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// ------------------------------------------------------------------ weight packs
// wf[(((g D + d) KK + tap) cg + c) 16 + n] = w[g og + n][c][d][tap] (n < og), else 0
__global__ __launch_bounds__(256) void pconv_pack_fwd(PShape s, long total, const float* __restrict__ w,
                                                      float* __restrict__ wf) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int n = (int)(idx & 15);
  long r = idx >> 4;
  const int c = (int)(r & (s.cg - 1));
  r >>= s.lcg;
  const int tap = (int)(r % s.KK);
  r /= s.KK;
  const int d = (int)(r % s.D);
  const int g = (int)(r / s.D);
  wf[idx] = n < s.og ? w[(((long)(g * s.og + n) * s.cg + c) * s.D + d) * s.KK + tap] : 0.f;
}

// wd[((g NT + nt) Kd + kk) 16 + nn] = w[g og + o][cl][d][tap] with kk = tap og + o, nt 16 + nn = d cg + cl; 0 outside
__global__ __launch_bounds__(256) void pconv_pack_dgrad(PShape s, int NT, int Kd, long total,
                                                        const float* __restrict__ w, float* __restrict__ wd) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int nn = (int)(idx & 15);
  long r = idx >> 4;
  const int kk = (int)(r % Kd);
  r /= Kd;
  const int nt = (int)(r % NT);
  const int g = (int)(r / NT);
  const int n = nt * 16 + nn;
  float v = 0.f;
  if (n < s.D * s.cg && kk < s.og * s.KK) {
    const int d = n >> s.lcg, cl = n & (s.cg - 1), tap = kk >> s.log, o = kk & (s.og - 1);
    v = w[(((long)(g * s.og + o) * s.cg + cl) * s.D + d) * s.KK + tap];
  }
  wd[idx] = v;
}

// ------------------------------------------------------------------ forward
// A block of 4 waves owns (2 samples, group, depth chunk): the chunk's planes of the group's channels sit in LDS
// [sample][depth][position][cg + 1]; a wave owns 32 positions of one sample (2 accumulators that share each B load).
// S = 1: y = bias + the sum; S > 1: the chunk's partial goes to part[chunk][row][O], summed by pconv_fwd_sum.
__global__ __launch_bounds__(256) void pconv_fwd_k(PShape s, int S, const float* __restrict__ x, long ldx,
                                                   const float* __restrict__ wf, const float* __restrict__ bias,
                                                   float* __restrict__ y, long ldy, float* __restrict__ part) {
  __shared__ float xs[PC_XS];
  const int bp = blockIdx.x, g = blockIdx.y, sp = blockIdx.z;
  const int cg = s.cg, cgp = cg + 1, chunk = pc_chunk(cg);
  const int d0 = sp * chunk, nd = min(chunk, s.D - d0);
  const int per = nd * 64 * cg;   // the group's floats of one sample's chunk
  if ((cg & 3) == 0) {
    for (int i = threadIdx.x * 4; i < 2 * per; i += 1024) {
      const int sm = i >= per, r = i - sm * per, c = r & (cg - 1), rp = r >> s.lcg, b = bp * 2 + sm;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (b < s.B) v = *reinterpret_cast<const f32x4*>(x + (((long)b * s.D + d0) * 64 + rp) * ldx + g * cg + c);
      float* o = xs + (sm * nd * 64 + rp) * cgp + c;
      o[0] = v[0], o[1] = v[1], o[2] = v[2], o[3] = v[3];
    }
  } else {
    for (int i = threadIdx.x; i < 2 * per; i += 256) {
      const int sm = i >= per, r = i - sm * per, c = r & (cg - 1), rp = r >> s.lcg, b = bp * 2 + sm;
      xs[(sm * nd * 64 + rp) * cgp + c] = b < s.B ? x[(((long)b * s.D + d0) * 64 + rp) * ldx + g * cg + c] : 0.f;
    }
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, m = lane & 15, kq = lane >> 4;
  const int sm = wave >> 1, b = bp * 2 + sm;
  if (b >= s.B) return;   // wave-uniform, after the only barrier
  const int tb = (wave & 1) * 2;                 // this wave's tiles tb, tb + 1: positions (tb + t) 16 + m
  const int h0 = tb * 2 + (m >> 3), w0 = m & 7;  // tile tb + 1 is 2 image rows further down
  const float* xw = xs + sm * nd * 64 * cgp;
  const int Kc = nd * cg, ksteps = (Kc + 3) >> 2;
  const float* wg = wf + ((long)g * s.D + d0) * s.KK * cg * 16;
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  // per kernel row the (kw, k-step) pairs are walked in groups of PC_U: every operand of a group is fetched before its
  // first MFMA, so the B loads' latency is paid once per group, not once per MFMA
  const int total = s.KS * ksteps;
  for (int kh = 0; kh < s.KS; ++kh) {
    const int hh0 = h0 + kh - s.ps, hh1 = hh0 + 2;
    const bool r0 = hh0 >= 0 && hh0 < 8, r1 = hh1 >= 0 && hh1 < 8;
    if (__ballot(r0 || r1) == 0) continue;
    int kw = 0, i = 0;
    for (int q0 = 0; q0 < total; q0 += PC_U) {
      float bv[PC_U], a0[PC_U], a1[PC_U];
      bool u0[PC_U], u1[PC_U];
#pragma unroll
      for (int j = 0; j < PC_U; ++j) {
        const bool in = q0 + j < total;   // uniform
        const int ww = w0 + kw - s.ps;
        const bool wok = in && ww >= 0 && ww < 8;
        const bool v0 = wok && r0, v1 = wok && r1;
        u0[j] = __ballot(v0) != 0;
        u1[j] = __ballot(v1) != 0;
        const int kk = 4 * i + kq, dl = kk >> s.lcg, c = kk & (cg - 1);
        const bool kin = kk < Kc && (u0[j] || u1[j]);
        bv[j] = kin ? wg[((long)(dl * s.KK + kh * s.KS + kw) * cg + c) * 16 + m] : 0.f;
        const int ao = (dl * 64 + hh0 * 8 + ww) * cgp + c;
        a0[j] = v0 && kin ? xw[ao] : 0.f;
        a1[j] = v1 && kin ? xw[ao + 16 * cgp] : 0.f;
        if (++i == ksteps) i = 0, ++kw;
      }
#pragma unroll
      for (int j = 0; j < PC_U; ++j) {
        if (u0[j]) acc0 = mfma4(a0[j], bv[j], acc0);
        if (u1[j]) acc1 = mfma4(a1[j], bv[j], acc1);
      }
    }
  }
  if (m >= s.og) return;
  const int o = g * s.og + m;
  const float bs = (S == 1 && bias) ? bias[o] : 0.f;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const f32x4 a = t ? acc1 : acc0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long row = (long)b * 64 + (tb + t) * 16 + kq * 4 + r;
      if (S == 1)
        y[row * ldy + o] = a[r] + bs;
      else
        part[((long)sp * s.B * 64 + row) * s.O + o] = a[r];
    }
  }
}

__global__ __launch_bounds__(256) void pconv_fwd_sum(int S, long rows, int O, const float* __restrict__ part,
                                                     const float* __restrict__ bias, float* __restrict__ y, long ldy) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows * O) return;
  const int o = (int)(idx % O);
  const long row = idx / O;
  float acc = bias ? bias[o] : 0.f;
  for (int sp = 0; sp < S; ++sp) acc += part[(long)sp * rows * O + idx];
  y[row * ldy + o] = acc;
}

// ------------------------------------------------------------------ data gradient
// A block owns (sample, group, 4 column tiles of 16 (depth, channel) pairs); the sample's 64 x og block of dy sits in
// LDS; a wave owns 16 positions and 4 accumulators that share each A value.  k = tap og + o walked in order.  wd: the
// packed weight, or (WLDS: a group's weight of up to PC_WLDS_FLOATS) w itself, which the block copies to LDS as it
// lies and reads element by element: no pack launch and no global latency in the loop, which is what the one-plane
// sites (D = 1, KS = 3: 36 k-steps) need to beat the direct kernel's single launch.
template <bool WLDS>
__global__ __launch_bounds__(256) void pconv_dgrad_k(PShape s, FastDiv ks, int NT, int Kd,
                                                     const float* __restrict__ dy, long lddy,
                                                     const float* __restrict__ wd, float* __restrict__ dx, long lddx,
                                                     float beta) {
  __shared__ float dys[64 * 17];
  __shared__ float wl[WLDS ? PC_WLDS_FLOATS : 1];
  const int b = blockIdx.x, g = blockIdx.y, nt0 = blockIdx.z * 4;
  const int og = s.og, ogp = og + 1;
  if constexpr (WLDS) {
    const int gsize = og * s.cg * s.D * s.KK;
    for (int i = threadIdx.x; i < gsize; i += 256) wl[i] = wd[(long)g * gsize + i];
  }
  for (int i = threadIdx.x; i < 64 * og; i += 256) {
    const int pos = i >> s.log, o = i & (og - 1);
    dys[pos * ogp + o] = dy[((long)b * 64 + pos) * lddy + g * og + o];
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, m = lane & 15, kq = lane >> 4;
  const int pos = wave * 16 + m, h = pos >> 3, w = pos & 7;
  const int Kreal = og * s.KK;
  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float* wb = wd + ((long)g * NT + nt0) * Kd * 16 + m;
  // groups of PC_U k-steps, operands first (see pconv_fwd_k), and two groups in flight: the next group's loads are
  // issued before this group's MFMAs (measured: it halves this kernel's time and does not pay in the forward)
  const int nsteps = Kd >> 2;
  struct Group {
    float a[PC_U], bw[PC_U][4];
    bool use[PC_U];
  };
  auto fetch = [&](int i0, Group& q) {
#pragma unroll
    for (int u = 0; u < PC_U; ++u) {
      const int kk = 4 * (i0 + u) + kq, tap = kk >> s.log, o = kk & (og - 1);
      int kw;
      const int kh = fdivmod(tap, ks, kw);
      const int hh = h + s.ps - kh, ww = w + s.ps - kw;
      const bool v = i0 + u < nsteps && kk < Kreal && hh >= 0 && hh < 8 && ww >= 0 && ww < 8;
      q.use[u] = __ballot(v) != 0;
      q.a[u] = v ? dys[(hh * 8 + ww) * ogp + o] : 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool on = q.use[u] && nt0 + j < NT;
        if constexpr (WLDS) {
          const int n = (nt0 + j) * 16 + m;
          const bool in = on && n < s.D * s.cg && kk < Kreal;
          q.bw[u][j] = in ? wl[((o * s.cg + (n & (s.cg - 1))) * s.D + (n >> s.lcg)) * s.KK + tap] : 0.f;
        } else {
          q.bw[u][j] = on ? wb[((long)j * Kd + kk) * 16] : 0.f;
        }
      }
    }
  };
  auto issue = [&](const Group& q) {
#pragma unroll
    for (int u = 0; u < PC_U; ++u) {
      if (!q.use[u]) continue;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (nt0 + j < NT) acc[j] = mfma4(q.a[u], q.bw[u][j], acc[j]);
    }
  };
  Group q0, q1;
  fetch(0, q0);
  for (int i0 = 0; i0 < nsteps; i0 += 2 * PC_U) {   // a group past the end fetches and issues nothing
    fetch(i0 + PC_U, q1);
    issue(q0);
    fetch(i0 + 2 * PC_U, q0);
    issue(q1);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int n = (nt0 + j) * 16 + m;
    if (nt0 + j >= NT || n >= s.D * s.cg) continue;
    const int d = n >> s.lcg, cl = n & (s.cg - 1);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float* out = dx + (((long)b * s.D + d) * 64 + wave * 16 + kq * 4 + r) * lddx + g * s.cg + cl;
      *out = (beta != 0.f ? beta * *out : 0.f) + acc[j][r];
    }
  }
}

// ------------------------------------------------------------------ weight gradient
// A block owns (group, column tile of 16 (depth, channel) pairs, kernel row kh, sample split z of SB); its 4 waves
// walk the samples z + SB (wave + 4 j) in order with one accumulator per kw (rows = the group's outputs, k = 4
// positions of one image row).  The waves are summed in wave order through LDS; SB > 1: the block's partial goes to
// part[z] in dw's layout and launch_sum_rows adds the splits in order.
__global__ __launch_bounds__(256) void pconv_wgrad_k(PShape s, int NT, int SB, const float* __restrict__ x, long ldx,
                                                     const float* __restrict__ dy, long lddy,
                                                     float* __restrict__ out) {
  __shared__ float red[4][9][256];
  const int g = blockIdx.x / NT, nt = blockIdx.x - g * NT, kh = blockIdx.y, z = blockIdx.z;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, m = lane & 15, kq = lane >> 4;
  const int n = nt * 16 + m;
  const bool nok = n < s.D * s.cg, aok = m < s.og;
  const int d = n >> s.lcg, cl = n & (s.cg - 1);
  f32x4 acc[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int b = z + SB * wave; b < s.B; b += 4 * SB) {
    const float* xb = x + (((long)b * s.D + (nok ? d : 0)) * 64) * ldx + g * s.cg + (nok ? cl : 0);
    const float* dyb = dy + (long)b * 64 * lddy + g * s.og + (aok ? m : 0);
    for (int i = 0; i < 16; ++i) {
      const int hh = (i >> 1) + kh - s.ps;   // positions 4 i .. 4 i + 3 share an image row
      if (hh < 0 || hh >= 8) continue;
      const int w = (i & 1) * 4 + kq;
      const float a = aok ? dyb[(long)(4 * i + kq) * lddy] : 0.f;
      float bv[9];
      bool use[9];
#pragma unroll
      for (int kw = 0; kw < 9; ++kw) {   // the row's operands first, then its MFMAs
        const int ww = w + kw - s.ps;
        const bool wok = kw < s.KS && ww >= 0 && ww < 8;
        use[kw] = __ballot(wok) != 0;
        bv[kw] = wok && nok ? xb[(long)(hh * 8 + ww) * ldx] : 0.f;
      }
#pragma unroll
      for (int kw = 0; kw < 9; ++kw)
        if (use[kw]) acc[kw] = mfma4(a, bv[kw], acc[kw]);
    }
  }
#pragma unroll
  for (int kw = 0; kw < 9; ++kw)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wave][kw][r * 64 + lane] = acc[kw][r];
  __syncthreads();
  const long wsize = (long)s.O * s.cg * s.D * s.KK;
  float* dst = out + (SB > 1 ? (long)z * wsize : 0);
  for (int i = threadIdx.x; i < s.KS * 256; i += 256) {
    const int kw = i >> 8, e = i & 255, r = e >> 6, ln = e & 63, o = (ln >> 4) * 4 + r, mm = ln & 15;
    const int nn = nt * 16 + mm;
    if (o >= s.og || nn >= s.D * s.cg) continue;
    const float t = ((red[0][kw][e] + red[1][kw][e]) + red[2][kw][e]) + red[3][kw][e];
    const int dd = nn >> s.lcg, cc = nn & (s.cg - 1);
    dst[((((long)(g * s.og + o) * s.cg + cc) * s.D + dd) * s.KS + kh) * s.KS + kw] = t;
  }
}

// db[o] = the column sum of dy: one block per output, a wave's xor tree, then the waves in order
__global__ __launch_bounds__(256) void pconv_db_k(long rows, const float* __restrict__ dy, long lddy,
                                                  float* __restrict__ db) {
  __shared__ float sh[4];
  const int o = blockIdx.x;
  float acc = 0.f;
  for (long r = threadIdx.x; r < rows; r += 256) acc += dy[r * lddy + o];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) db[o] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

int ilog2(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return (1 << l) == v ? l : -1;
}

bool shape_ok(int D, int C, int O, int G, int KS, long ldx, long ldy) {
  if (D < 1 || D > 4096 || C < 1 || O < 1 || G < 1 || KS < 3 || KS > 9 || !(KS & 1)) return false;
  if (C % G || O % G || C % 16) return false;   // the model's few-channel LiDAR conv1 stays on the direct family
  const int cg = C / G, og = O / G;
  if (cg < 2 || cg > 32 || ilog2(cg) < 0 || og < 2 || og > 16 || ilog2(og) < 0) return false;
  if (G > 65535 || ldx < C || ldy < O || (ldx & 3) || (ldy & 3)) return false;
  return true;
}

PShape make_shape(int B, int D, int C, int O, int G, int KS) {
  const int cg = C / G, og = O / G;
  return PShape{B, D, C, O, G, KS, cg, og, ilog2(cg), ilog2(og), KS * KS, KS / 2};
}

struct PSizes {
  long packF, partF, packD, partW, wsize;
  int S, NT, Kd, SB;
};

PSizes sizes(int B, int D, int C, int O, int G, int KS) {
  const int cg = C / G, og = O / G, KK = KS * KS;
  PSizes z;
  z.S = vc_cdiv(D, pc_chunk(cg));
  z.packF = (long)D * KK * C * 16;
  z.partF = z.S > 1 ? (long)z.S * B * 64 * O : 0;
  z.NT = vc_cdiv((long)D * cg, 16);
  z.Kd = (og * KK + 3) & ~3;
  z.packD = (long)G * z.NT * z.Kd * 16;
  z.wsize = (long)O * cg * D * KK;
  const long blocks0 = (long)G * z.NT * KS;
  z.SB = (int)std::min<long>(vc_cdiv(B, 4), std::max<long>(1, 512 / blocks0));
  z.partW = z.SB > 1 ? z.SB * z.wsize : 0;
  return z;
}

long ws_need(const PSizes& z) { return std::max(std::max(z.packF + z.partF, z.packD), std::max<long>(z.partW, 1)); }

// the checks every entry point shares: shape, strides, sizes that index in 32 bits, alignment, workspace
int pconv_check(int B, int D, int C, int O, int G, int KS, const void* xs, long ldx, const void* ys, long ldy,
                const void* ws, long ws_floats) {
  VC_REQUIRE(B > 0 && shape_ok(D, C, O, G, KS, ldx, ldy));
  VC_REQUIRE_I32((long)B * D * 64 * ldx);
  VC_REQUIRE_I32((long)B * 64 * ldy);
  const PSizes z = sizes(B, D, C, O, G, KS);
  VC_REQUIRE_I32(ws_need(z));
  VC_REQUIRE(vc_cdiv(B, 2) <= 65535 * 32768 && z.S <= 65535 && z.NT <= 65535 * 4);
  VC_REQUIRE(xs && ys && ws && ws_floats >= ws_need(z));
  VC_REQUIRE(((uintptr_t)xs & 15) == 0 && ((uintptr_t)ys & 15) == 0 && ((uintptr_t)ws & 15) == 0);
  return VC_OK;
}

}  // namespace

VC_API int vc_mhst_pconv_ok(int D, int C, int O, int G, int KS, long ldx, long ldy) {
  return shape_ok(D, C, O, G, KS, ldx, ldy) ? 1 : 0;
}

VC_API int vc_mhst_pconv_ws_floats(int B, int D, int C, int O, int G, int KS) {
  if (B <= 0 || !shape_ok(D, C, O, G, KS, C + (-C & 3), O + (-O & 3))) return -1;
  const long n = ws_need(sizes(B, D, C, O, G, KS));
  return n < (1L << 31) ? (int)n : -1;
}

VC_API int vc_mhst_pconv_fwd(int B, int D, int C, int O, int G, int KS, const float* x, long ldx, const float* w,
                             const float* bias, float* y, long ldy, float* ws, long ws_floats, hipStream_t stream) {
  if (pconv_check(B, D, C, O, G, KS, x, ldx, y, ldy, ws, ws_floats)) return VC_EINVAL;
  VC_REQUIRE(w);
  const PShape s = make_shape(B, D, C, O, G, KS);
  const PSizes z = sizes(B, D, C, O, G, KS);
  float* part = ws + z.packF;
  hipLaunchKernelGGL(pconv_pack_fwd, dim3(vc_cdiv(z.packF, 256)), dim3(256), 0, stream, s, z.packF, w, ws);
  VC_CHECK_LAUNCH();
  hipLaunchKernelGGL(pconv_fwd_k, dim3(vc_cdiv(B, 2), G, z.S), dim3(256), 0, stream, s, z.S, x, ldx, ws, bias, y, ldy,
                     part);
  VC_CHECK_LAUNCH();
  if (z.S > 1) {
    const long rows = (long)B * 64;
    hipLaunchKernelGGL(pconv_fwd_sum, dim3(vc_cdiv(rows * O, 256)), dim3(256), 0, stream, z.S, rows, O, part, bias, y,
                       ldy);
    VC_CHECK_LAUNCH();
  }
  return VC_OK;
}

VC_API int vc_mhst_pconv_dgrad(int B, int D, int C, int O, int G, int KS, const float* dy, long lddy, const float* w,
                               float* dx, long lddx, float beta, float* ws, long ws_floats, hipStream_t stream) {
  if (pconv_check(B, D, C, O, G, KS, dx, lddx, dy, lddy, ws, ws_floats)) return VC_EINVAL;
  VC_REQUIRE(w && B <= 65535 * 32768);
  const PShape s = make_shape(B, D, C, O, G, KS);
  const PSizes z = sizes(B, D, C, O, G, KS);
  const dim3 grid(B, G, vc_cdiv(z.NT, 4));
  if (z.wsize / G <= PC_WLDS_FLOATS) {
    hipLaunchKernelGGL(pconv_dgrad_k<true>, grid, dim3(256), 0, stream, s, make_fastdiv(KS), z.NT, z.Kd, dy, lddy, w, dx,
                       lddx, beta);
  } else {
    hipLaunchKernelGGL(pconv_pack_dgrad, dim3(vc_cdiv(z.packD, 256)), dim3(256), 0, stream, s, z.NT, z.Kd, z.packD, w,
                       ws);
    VC_CHECK_LAUNCH();
    hipLaunchKernelGGL(pconv_dgrad_k<false>, grid, dim3(256), 0, stream, s, make_fastdiv(KS), z.NT, z.Kd, dy, lddy, ws,
                       dx, lddx, beta);
  }
  VC_CHECK_LAUNCH();
  return VC_OK;
}

VC_API int vc_mhst_pconv_wgrad(int B, int D, int C, int O, int G, int KS, const float* x, long ldx, const float* dy,
                               long lddy, float* dw, float* db, float* ws, long ws_floats, hipStream_t stream) {
  if (pconv_check(B, D, C, O, G, KS, x, ldx, dy, lddy, ws, ws_floats)) return VC_EINVAL;
  VC_REQUIRE(dw);
  const PShape s = make_shape(B, D, C, O, G, KS);
  const PSizes z = sizes(B, D, C, O, G, KS);
  VC_REQUIRE_I32((long)G * z.NT);
  hipLaunchKernelGGL(pconv_wgrad_k, dim3(G * z.NT, KS, z.SB), dim3(256), 0, stream, s, z.NT, z.SB, x, ldx, dy, lddy,
                     z.SB > 1 ? ws : dw);
  VC_CHECK_LAUNCH();
  if (z.SB > 1 && launch_sum_rows(z.SB, (int)z.wsize, ws, z.wsize, 0, dw, 0.f, stream)) return VC_EINVAL;
  if (db) {
    hipLaunchKernelGGL(pconv_db_k, dim3(O), dim3(256), 0, stream, (long)B * 64, dy, lddy, db);
    VC_CHECK_LAUNCH();
  }
  return VC_OK;
}

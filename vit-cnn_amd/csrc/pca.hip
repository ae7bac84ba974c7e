// Principal-component analysis of the HSI cube's pixel spectra on the device (vitcnn_amd/pca.py; the reference's
// utils.py:85-93 applyPCA runs scikit-learn on the host).  Operands are the rows of an [n, C] fp32 matrix with leading
// dimension ld >= C -- the [W, H, C] cube with n = W * H.
//   vc_pca_mean     column means in fp64: per-slab partial rows, then a fixed-order sum over the slabs
//   vc_pca_cov      sum_rows xc xc^T / (n - 1), xc = x - mean32: a SYRK on the fp32 MFMA over upper-triangle pairs of
//                   64-column tiles x slabs of vc_pca_slab_rows() rows, one fp32 tile partial per (slab, pair), then the
//                   slabs summed in fp64 in a fixed order and mirrored
//   vc_pca_project  y = (x - mean32) wt on the fp32 MFMA, one pass over x with wt in LDS
// No floating-point atomics anywhere: a second call gives the same bits.
#include "mfma_tiles.h"

namespace pca {

constexpr int MAXC = 512, MAXK = 64;
constexpr int SLAB = 2048;        // R: rows one block of the covariance accumulates in fp32 (two fma chains of R / 2)
constexpr int TILE = 64;          // columns per covariance tile
constexpr int TILE_FLOATS = TILE * TILE;
constexpr int MEAN_SLABS = 1024;  // at most this many partial rows of the mean (at least 256 rows each)

static inline long mean_rows(long n) { return std::max(256L, (n + MEAN_SLABS - 1) / MEAN_SLABS); }
static inline long mean_slabs(long n) { return (n + mean_rows(n) - 1) / mean_rows(n); }
static inline long cov_slabs(long n) { return (n + SLAB - 1) / SLAB; }
static inline int cov_tiles(int C) { return (C + TILE - 1) / TILE; }
static inline int cov_pairs(int C) { return cov_tiles(C) * (cov_tiles(C) + 1) / 2; }

static inline bool shape_ok(long n, int C, long ld) {
  return n >= 2 && n < (1L << 31) - 64 && C >= 1 && C <= MAXC && ld >= C;
}

// ---------------------------------------------------------------------------------------------------- mean
// part[slab][c] = sum of column c over the slab's rows.  A thread owns 4 adjacent columns (one 16-B load per row where
// the operand allows it) and every (256 / lanes4)-th row of the slab, in ascending order; the row lanes are then
// combined in a fixed order.  lanes4 = ceil(C / 4) <= 128, so a row is one contiguous run of the block's loads.
static __global__ __launch_bounds__(256) void mean_partial_kernel(long n, int C, long ld, const float* __restrict__ x,
                                                                   long rows, int lanes4, int vec,
                                                                   double* __restrict__ part) {
  __shared__ double sh[256][4];
  const int nrl = 256 / lanes4;   // row lanes
  const int cl = threadIdx.x % lanes4, rl = threadIdx.x / lanes4, c = 4 * cl;
  const long r0 = (long)blockIdx.x * rows, r1 = min(n, r0 + rows);
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  if (rl < nrl) {
    if (vec && c + 3 < C) {
#pragma unroll 4
      for (long r = r0 + rl; r < r1; r += nrl) {
        const float4 q = *reinterpret_cast<const float4*>(x + r * ld + c);
        s[0] += (double)q.x;
        s[1] += (double)q.y;
        s[2] += (double)q.z;
        s[3] += (double)q.w;
      }
    } else {
      for (long r = r0 + rl; r < r1; r += nrl) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (c + j < C) s[j] += (double)x[r * ld + c + j];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) sh[threadIdx.x][j] = s[j];
  __syncthreads();
  if (rl == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (c + j < C) {
        double v = 0.0;
        for (int q = 0; q < nrl; ++q) v += sh[q * lanes4 + cl][j];
        part[(long)blockIdx.x * C + c + j] = v;
      }
  }
}

// mean[c] = (sum over the slabs of part[slab][c]) / n: 16 columns x 16 slab lanes, fixed-order combine
static __global__ __launch_bounds__(256) void mean_final_kernel(long n, int C, int slabs, const double* __restrict__ part,
                                                                 double* __restrict__ mean) {
  __shared__ double sh[16][17];
  const int cl = threadIdx.x & 15, pl = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cl;
  double s = 0.0;
  if (c < C)
    for (int p = pl; p < slabs; p += 16) s += part[(long)p * C + c];
  sh[pl][cl] = s;
  __syncthreads();
  if (pl == 0 && c < C) {
    double v = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) v += sh[i][cl];
    mean[c] = v / (double)n;
  }
}

// ---------------------------------------------------------------------------------------------- covariance
typedef g2::Stage<false, true, TILE, false> Panel;   // element (column r, row k) of x at x[k * ld + r]

// pair index -> tiles (ti <= tj), pairs numbered row by row of the upper triangle
__device__ __forceinline__ void pair_tiles(int pair, int tiles, int& ti, int& tj) {
  ti = 0;
  while (pair >= tiles - ti) {
    pair -= tiles - ti;
    ++ti;
  }
  tj = ti + pair;
}

// xc = x - mean32 on the staged registers: only where the element is a real one (row < kend, column < C), so rows past
// n and columns past C stay exactly zero.  A thread's 4 columns are the same for every piece of the panel.
__device__ __forceinline__ void centre(Panel& s, const float (&mu)[4], int col, int C, int k0, int kend, int tid) {
#pragma unroll
  for (int i = 0; i < Panel::NR / 4; ++i) {
    const int k = k0 + (tid + 256 * i) / (TILE / 4);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (k < kend && col + j < C) s.raw[4 * i + j] -= mu[j];
  }
}

// One block: the 64 x 64 tile (ti, tj) of sum_k xc[k][i] xc[k][j] over the slab's rows, 4 waves of 32 x 32, k-tiles of 32
// rows through two LDS stages (the next tile's global loads fly behind the current tile's MFMAs).  A diagonal pair
// stages one panel and reads it as both operands.
static __global__ __launch_bounds__(256) void cov_partial_kernel(long n, int C, long ld, const float* __restrict__ x,
                                                                  const float* __restrict__ mean32, int tiles, int pairs,
                                                                  float* __restrict__ part, int vec) {
  constexpr int PANEL = TILE * g2::ROWB, STAGE = 2 * PANEL, KT = Panel::KT;
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int pair = blockIdx.x % pairs;
  const long slab = blockIdx.x / pairs;
  int ti, tj;
  pair_tiles(pair, tiles, ti, tj);
  const bool diag = ti == tj;
  const long kbeg = slab * SLAB;
  const int kend = (int)(min(n, kbeg + SLAB) - kbeg);   // rows of this slab, k counted from its first row
  const float* xs = x + kbeg * ld;
  const int i0 = ti * TILE, j0 = tj * TILE;
  const int ci = i0 + 4 * (tid % (TILE / 4)), cj = j0 + 4 * (tid % (TILE / 4));
  float mi[4], mj[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    mi[j] = ci + j < C ? mean32[ci + j] : 0.f;
    mj[j] = cj + j < C ? mean32[cj + j] : 0.f;
  }

  Panel sa, sb;
  f32x4 acc[2][2][2];
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[c][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = (kend + KT - 1) / KT;
  sa.load(xs, ld, C, i0, 0, kend, false, vec != 0, tid);
  centre(sa, mi, ci, C, 0, kend, tid);
  sa.store(smem, tid);
  if (!diag) {
    sb.load(xs, ld, C, j0, 0, kend, false, vec != 0, tid);
    centre(sb, mj, cj, C, 0, kend, tid);
    sb.store(smem + PANEL, tid);
  }
  __syncthreads();
  for (int t = 0; t < nk; ++t) {
    char* cur = smem + (t & 1) * STAGE;
    char* nxt = smem + ((t & 1) ^ 1) * STAGE;
    const int k1 = (t + 1) * KT;
    if (t + 1 < nk) {
      sa.load(xs, ld, C, i0, k1, kend, false, vec != 0, tid);
      if (!diag) sb.load(xs, ld, C, j0, k1, kend, false, vec != 0, tid);
    }
    g2::mma_ktile<false, 2, 2, Panel, Panel, 2>(cur, diag ? cur : cur + PANEL, wm * 32, wn * 32, lane, acc);
    if (t + 1 < nk) {
      centre(sa, mi, ci, C, k1, kend, tid);
      sa.store(nxt, tid);
      if (!diag) {
        centre(sb, mj, cj, C, k1, kend, tid);
        sb.store(nxt + PANEL, tid);
      }
    }
    __syncthreads();
  }

  // C/D map of the 16x16 MFMAs: col = lane & 15, row = (lane >> 4) * 4 + r.  The whole tile is written (columns past C
  // hold zeros), so the second launch reads no stale workspace.
  float* out = part + (long)blockIdx.x * TILE_FLOATS;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = wm * 32 + a * 16 + (lane >> 4) * 4 + r;
        const int nn = wn * 32 + b * 16 + (lane & 15);
        out[m * TILE + nn] = acc[0][a][b][r] + acc[1][a][b][r];
      }
}

// cov[i][j] = cov[j][i] = (sum over the slabs, in a fixed order in fp64, of the tile partials) / (n - 1): 16 tile
// elements x 16 slab lanes per block.  A diagonal tile takes its upper half only, so the result is exactly symmetric.
static __global__ __launch_bounds__(256) void cov_final_kernel(long n, int C, int tiles, int pairs, int slabs,
                                                                const float* __restrict__ part, double* __restrict__ cov) {
  __shared__ double sh[16][17];
  const int el = threadIdx.x & 15, pl = threadIdx.x >> 4;
  constexpr int BPT = TILE_FLOATS / 16;   // blocks per tile
  const int pair = blockIdx.x / BPT, e = (blockIdx.x % BPT) * 16 + el;
  int ti, tj;
  pair_tiles(pair, tiles, ti, tj);
  const int m = e / TILE, nn = e % TILE;
  const int i = ti * TILE + m, j = tj * TILE + nn;
  const bool valid = i < C && j < C && (ti < tj || m <= nn);
  double s = 0.0;
  if (valid)
    for (int p = pl; p < slabs; p += 16) s += (double)part[((long)p * pairs + pair) * TILE_FLOATS + e];
  sh[pl][el] = s;
  __syncthreads();
  if (pl == 0 && valid) {
    double v = 0.0;
#pragma unroll
    for (int q = 0; q < 16; ++q) v += sh[q][el];
    v /= (double)(n - 1);
    cov[(long)i * C + j] = v;
    cov[(long)j * C + i] = v;
  }
}

// ---------------------------------------------------------------------------------------------- projection
// y[i][k] = sum_c (x[i][c] - mean32[c]) wt[c][k] on the fp32 MFMA.  wt sits in LDS for the whole launch: rows c up to
// the next multiple of 32, KP = 32 or 64 columns, rows past C and columns past K zero, 16-column blocks XOR-swizzled by
// (c >> 2) & 1 so that the four k-rows a fragment read touches fall on distinct banks.  A block walks tiles of 64 rows
// of x; a tile's 32-column pieces are staged K-contiguous (g2::Stage, centred in registers) through two LDS stages;
// wave w owns rows 16 w .. 16 w + 15 and all NT = ceil(K / 16) column tiles: one accumulator chain of C per output.
typedef g2::Stage<false, false, 64, false> Rows;   // element (row r, column k) of x at x[r * ld + k]

__device__ __forceinline__ void centre_rows(Rows& s, const float* __restrict__ mean32, int n, int row0, int c0, int C,
                                            int tid) {
  const int k = c0 + (tid & 7) * 4;
  float mu[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) mu[j] = k + j < C ? mean32[k + j] : 0.f;
#pragma unroll
  for (int i = 0; i < Rows::NR / 4; ++i) {
    const int r = row0 + (tid >> 3) + 32 * i;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (r < n && k + j < C) s.raw[4 * i + j] -= mu[j];
  }
}

template <int NT, int WTF>
static __global__ __launch_bounds__(256) void project_kernel(int n, int C, long ld, int K, const float* __restrict__ x,
                                                              const float* __restrict__ mean32,
                                                              const float* __restrict__ wt, float* __restrict__ y,
                                                              long ldy, int tiles, int vec) {
  constexpr int KP = NT <= 2 ? 32 : 64, KT = Rows::KT, STAGE = 64 * g2::ROWB;
  __shared__ __attribute__((aligned(16))) float wts[WTF];
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, l16 = lane & 15;
  const int CP = (C + KT - 1) / KT * KT;
  for (int e = tid; e < CP * KP; e += 256) {
    const int c = e / KP, k = (e % KP) ^ (((c >> 2) & 1) << 4);
    wts[e] = (c < C && k < K) ? wt[(long)c * K + k] : 0.f;
  }
  const int nk = CP / KT;
  int bcol[NT];   // the lane's swizzled columns: every k-row c it reads has (c >> 2) & 1 = g & 1
#pragma unroll
  for (int ni = 0; ni < NT; ++ni) bcol[ni] = (16 * ni + l16) ^ ((g & 1) << 4);
  Rows sa;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int i0 = tile * 64;
    f32x4 acc[NT];
#pragma unroll
    for (int ni = 0; ni < NT; ++ni) acc[ni] = f32x4{0.f, 0.f, 0.f, 0.f};
    sa.load(x, ld, n, i0, 0, C, false, vec != 0, tid);
    centre_rows(sa, mean32, n, i0, 0, C, tid);
    __syncthreads();   // the previous tile's last piece has been read (first tile: wts is complete)
    sa.store(smem, tid);
    __syncthreads();
    for (int t = 0; t < nk; ++t) {
      const char* cur = smem + (t & 1) * STAGE;
      char* nxt = smem + ((t & 1) ^ 1) * STAGE;
      if (t + 1 < nk) sa.load(x, ld, n, i0, (t + 1) * KT, C, false, vec != 0, tid);
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const uint4 a = Rows::frag(cur, 16 * wave, s, lane);
        const float* w = wts + (t * KT + 16 * s + 4 * g) * KP;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int ni = 0; ni < NT; ++ni)
            acc[ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a[j]), w[j * KP + bcol[ni]], acc[ni], 0, 0, 0);
      }
      if (t + 1 < nk) {
        centre_rows(sa, mean32, n, i0, (t + 1) * KT, C, tid);
        sa.store(nxt, tid);
      }
      __syncthreads();
    }
    // C/D map of the 16x16 MFMAs: col = lane & 15, row = (lane >> 4) * 4 + r
#pragma unroll
    for (int ni = 0; ni < NT; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + 16 * wave + 4 * g + r, k = 16 * ni + l16;
        if (i < n && k < K) y[(long)i * ldy + k] = acc[ni][r];
      }
  }
}

template <int NT>
static int launch_project(long n, int C, long ld, int K, const float* x, const float* mean32, const float* wt, float* y,
                          long ldy, int vec, hipStream_t stream) {
  const int tiles = (int)((n + 63) / 64);
  constexpr int KP = NT <= 2 ? 32 : 64;
  if ((C + 31) / 32 * 32 * KP <= 8192) {
    const int grid = std::min(tiles, 768);   // 48 KB of LDS: three blocks per CU
    hipLaunchKernelGGL((project_kernel<NT, 8192>), dim3(grid), dim3(256), 0, stream, (int)n, C, ld, K, x, mean32, wt, y,
                       ldy, tiles, vec);
  } else {
    const int grid = std::min(tiles, 256);   // up to 128 KB of wt: one block per CU
    hipLaunchKernelGGL((project_kernel<NT, MAXC * MAXK>), dim3(grid), dim3(256), 0, stream, (int)n, C, ld, K, x, mean32,
                       wt, y, ldy, tiles, vec);
  }
  VC_CHECK_LAUNCH();
  return VC_OK;
}

}  // namespace pca

VC_EXPORT int vc_pca_slab_rows(void) { return pca::SLAB; }

VC_EXPORT int vc_pca_cov_workspace(long n, int C, long* bytes) {
  VC_REQUIRE(pca::shape_ok(n, C, C) && bytes);
  const long mean_b = pca::mean_slabs(n) * C * (long)sizeof(double);
  const long cov_b = pca::cov_slabs(n) * pca::cov_pairs(C) * pca::TILE_FLOATS * (long)sizeof(float);
  *bytes = std::max(mean_b, cov_b);
  return VC_OK;
}

VC_EXPORT int vc_pca_mean(long n, int C, long ld, const float* x, void* workspace, double* mean, hipStream_t stream) {
  VC_REQUIRE(pca::shape_ok(n, C, ld));
  VC_REQUIRE(x && workspace && mean && (uintptr_t)workspace % 8 == 0);
  const long rows = pca::mean_rows(n);
  const int slabs = (int)pca::mean_slabs(n);
  double* part = static_cast<double*>(workspace);
  const int vec = (uintptr_t)x % 16 == 0 && ld % 4 == 0;
  hipLaunchKernelGGL(pca::mean_partial_kernel, dim3(slabs), dim3(256), 0, stream, n, C, ld, x, rows, (C + 3) / 4, vec,
                     part);
  VC_CHECK_LAUNCH();
  hipLaunchKernelGGL(pca::mean_final_kernel, dim3(vc_cdiv(C, 16)), dim3(256), 0, stream, n, C, slabs, part, mean);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

VC_EXPORT int vc_pca_cov(long n, int C, long ld, const float* x, const float* mean32, void* workspace, double* cov,
                         hipStream_t stream) {
  VC_REQUIRE(pca::shape_ok(n, C, ld));
  VC_REQUIRE(x && mean32 && workspace && cov && (uintptr_t)workspace % 16 == 0);
  const int tiles = pca::cov_tiles(C), pairs = pca::cov_pairs(C);
  const long slabs = pca::cov_slabs(n);
  VC_REQUIRE_I32(slabs * pairs);
  VC_REQUIRE_I32((long)pairs * (pca::TILE_FLOATS / 16));
  const int vec = (uintptr_t)x % 16 == 0 && ld % 4 == 0;
  float* part = static_cast<float*>(workspace);
  hipLaunchKernelGGL(pca::cov_partial_kernel, dim3((unsigned)(slabs * pairs)), dim3(256), 0, stream, n, C, ld, x, mean32,
                     tiles, pairs, part, vec);
  VC_CHECK_LAUNCH();
  hipLaunchKernelGGL(pca::cov_final_kernel, dim3(pairs * (pca::TILE_FLOATS / 16)), dim3(256), 0, stream, n, C, tiles,
                     pairs, (int)slabs, part, cov);
  VC_CHECK_LAUNCH();
  return VC_OK;
}

VC_EXPORT int vc_pca_project(long n, int C, long ld, int K, const float* x, const float* mean32, const float* wt,
                             float* y, long ldy, hipStream_t stream) {
  VC_REQUIRE(pca::shape_ok(n, C, ld));
  VC_REQUIRE(K >= 1 && K <= std::min(C, pca::MAXK) && ldy >= K);
  VC_REQUIRE(x && mean32 && wt && y);
  const int vec = (uintptr_t)x % 16 == 0 && ld % 4 == 0;
  switch ((K + 15) / 16) {   // 16-column output tiles per wave
    case 1: return pca::launch_project<1>(n, C, ld, K, x, mean32, wt, y, ldy, vec, stream);
    case 2: return pca::launch_project<2>(n, C, ld, K, x, mean32, wt, y, ldy, vec, stream);
    case 3: return pca::launch_project<3>(n, C, ld, K, x, mean32, wt, y, ldy, vec, stream);
    default: return pca::launch_project<4>(n, C, ld, K, x, mean32, wt, y, ldy, vec, stream);
  }
}

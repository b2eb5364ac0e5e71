// quality.hip -- PSNR and SSIM sums of image pairs, in fp64: per plane of two (rows, C, H, W) sets a and b
//   out[plane] = [ sum (a - b)^2,  sum |a - b|,  pixels counted,  sum of the windows' SSIM,  windows counted ]
// over the pixels of a region (an H x W mask per image, or every pixel) and over the K x K windows whose centre pixel lies in it,
// and optionally every window's SSIM.  One launch, one workgroup per plane: the plane is read once, widened exactly (u8 or fp32 to
// fp32 in LDS, 32 KB for the largest pair of planes, to fp64 when it is used), and five numbers leave.
// A window's five weighted moments are summed directly from the LDS-resident plane, a row at a time: h = sum_s win[s] p[i + r][j + s]
// in ascending s from zero, then m = sum_r win[r] h_r in ascending r from zero, every step one fma.  The products a a, b b and a b
// are exact in fp64 (24 x 24 or 8 x 8 bits) and go through the SAME chain in the same operand order, so for a == b the three second
// moments, and with them the variances and the covariance, are equal bit for bit: the device manifold.hip uses for its norms.
// The rational itself is compiled without contraction: 2 m m and m m + m m, 2 v and v + v are then the same doubles and a == b
// gives ssim == 1.0 exactly in every window.
// The sums: a thread adds its pixels (its windows) in index order, a shuffle tree adds the lanes of a wave, the four waves are
// added in wave order.  No atomics, no workspace, nothing depends on the order in which workgroups run: the same arguments give the
// same bits.  A pixel outside the region is never added (a select, not a product): a NaN there stays out of the pixel sums.
#include "common.h"

#pragma clang fp contract(off)

namespace afd {

constexpr int kQMax = 64;                          // largest H and W
constexpr int kQThreads = 256;
constexpr int kQPer = kQMax * kQMax / kQThreads;   // pixels of a plane per thread
constexpr int kQMaxK = 15;
constexpr int kQOut = 5;
constexpr int kQCommonK = 11;                      // the window every paper uses gets a kernel of its own

struct QWin { double w[kQMaxK]; };                 // the window travels as a kernel argument (no H2D copy)

// KT: the window size known at compile time (the taps of a row unrolled, the weights in scalar registers), or 0 for any K.  Both
// forms run the same operations in the same order.
template <bool U8, int KT>
__global__ __launch_bounds__(kQThreads) void pair_quality_k(const void* __restrict__ a, const void* __restrict__ b, int C, int H, int W, QWin win,
                                                            int K_any, double c1, double c2, const uint8_t* __restrict__ region, int region_shared,
                                                            double* __restrict__ out, double* __restrict__ ssim_map) {
  __shared__ float sa[kQMax * kQMax], sb[kQMax * kQMax];
  __shared__ double red[(kQThreads / kWave) * kQOut];
  const int tid = threadIdx.x, K = KT ? KT : K_any;
  const long plane = blockIdx.x;
  const int HW = H * W, Wo = W - K + 1, NW = (H - K + 1) * Wo, half = (K - 1) >> 1;
  const uint8_t* reg = region ? region + (region_shared ? 0 : plane / C) * HW : nullptr;
  const long base = plane * HW;
  double v[kQOut] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int j = 0; j < kQPer; ++j) {
    const int e = tid + kQThreads * j;
    if (e < HW) {
      const float x = U8 ? (float)static_cast<const uint8_t*>(a)[base + e] : static_cast<const float*>(a)[base + e];
      const float y = U8 ? (float)static_cast<const uint8_t*>(b)[base + e] : static_cast<const float*>(b)[base + e];
      sa[e] = x;
      sb[e] = y;
      if (!reg || reg[e]) {
        const double d = (double)x - (double)y;
        v[0] += d * d;
        v[1] += fabs(d);
        v[2] += 1.0;
      }
    }
  }
  __syncthreads();
  double* map = ssim_map ? ssim_map + plane * NW : nullptr;
  for (int e = tid; e < NW; e += kQThreads) {
    const int i = e / Wo, j = e - i * Wo;
    double ma = 0.0, mb = 0.0, maa = 0.0, mbb = 0.0, mab = 0.0;
    for (int r = 0; r < K; ++r) {
      const float* pa = sa + (i + r) * W + j;
      const float* pb = sb + (i + r) * W + j;
      double ha = 0.0, hb = 0.0, haa = 0.0, hbb = 0.0, hab = 0.0;
#pragma unroll
      for (int s = 0; s < K; ++s) {
        const double x = (double)pa[s], y = (double)pb[s], ws = win.w[s];
        ha = fma(ws, x, ha);
        hb = fma(ws, y, hb);
        haa = fma(ws, x * x, haa);
        hbb = fma(ws, y * y, hbb);
        hab = fma(ws, x * y, hab);
      }
      const double wr = win.w[r];
      ma = fma(wr, ha, ma);
      mb = fma(wr, hb, mb);
      maa = fma(wr, haa, maa);
      mbb = fma(wr, hbb, mbb);
      mab = fma(wr, hab, mab);
    }
    const double vaa = maa - ma * ma, vbb = mbb - mb * mb, vab = mab - ma * mb;
    const double ssim = ((2.0 * ma * mb + c1) * (2.0 * vab + c2)) / ((ma * ma + mb * mb + c1) * (vaa + vbb + c2));
    if (map) map[e] = ssim;
    if (!reg || reg[(i + half) * W + j + half]) {
      v[3] += ssim;
      v[4] += 1.0;
    }
  }
#pragma unroll
  for (int k = 0; k < kQOut; ++k)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_down(v[k], o, kWave);
  if ((tid & 63) == 0)
#pragma unroll
    for (int k = 0; k < kQOut; ++k) red[(tid >> 6) * kQOut + k] = v[k];
  __syncthreads();
  if (tid < kQOut) out[plane * kQOut + tid] = ((red[tid] + red[kQOut + tid]) + red[2 * kQOut + tid]) + red[3 * kQOut + tid];
}

}  // namespace afd
using namespace afd;

template <bool U8>
static int launch_pair_quality(const char* name, const void* a, const void* b, long planes, int C, int H, int W, const double* win, int K, double c1,
                               double c2, const uint8_t* region, long region_rows, double* out, double* ssim_map, hipStream_t st) {
  AFD_REQUIRE(a && b && win && out, "%s: a, b, win and out must not be NULL", name);
  AFD_REQUIRE(planes > 0 && C > 0, "%s: planes and C must be positive (got %ld, %d)", name, planes, C);
  AFD_REQUIRE(planes % C == 0, "%s: planes must be a multiple of C (got %ld, %d)", name, planes, C);
  AFD_REQUIRE(planes < (1L << 31), "%s: planes must be below 2^31 (got %ld)", name, planes);
  AFD_REQUIRE(H >= 1 && H <= kQMax && W >= 1 && W <= kQMax, "%s: H and W must lie in [1, %d] (got %d, %d)", name, kQMax, H, W);
  AFD_REQUIRE(K >= 1 && K <= kQMaxK && (K & 1), "%s: K must be odd and lie in [1, %d] (got %d)", name, kQMaxK, K);
  AFD_REQUIRE(K <= H && K <= W, "%s: K must be at most min(H, W) (got K = %d, H = %d, W = %d)", name, K, H, W);
  AFD_REQUIRE(region_rows == 1 || region_rows == planes / C, "%s: region_rows must be 1 or planes / C = %ld (got %ld)", name, planes / C,
              region_rows);
  AFD_REQUIRE(((uintptr_t)out & 7) == 0, "%s: out must be 8-byte aligned", name);
  AFD_REQUIRE(((uintptr_t)ssim_map & 7) == 0, "%s: ssim_map must be 8-byte aligned", name);
  AFD_REQUIRE(U8 || ((uintptr_t)a & 3) == 0, "%s: a must be 4-byte aligned", name);
  AFD_REQUIRE(U8 || ((uintptr_t)b & 3) == 0, "%s: b must be 4-byte aligned", name);
  const long ib = planes * H * W * (U8 ? 1 : 4), ob = planes * kQOut * 8, mb = planes * (H - K + 1) * (W - K + 1) * 8;
  struct { const void* p; long bytes; const char* what; } in[] = {{a, ib, "a"}, {b, ib, "b"}, {region, region_rows * H * W, "region"}};
  for (const auto& i : in)
    AFD_REQUIRE(!overlaps(out, ob, i.p, i.bytes) && !(ssim_map && overlaps(ssim_map, mb, i.p, i.bytes)), "%s: out and ssim_map must not overlap %s",
                name, i.what);
  AFD_REQUIRE(!(ssim_map && overlaps(ssim_map, mb, out, ob)), "%s: out and ssim_map must not overlap each other", name);
  QWin qw;
  for (int k = 0; k < kQMaxK; ++k) qw.w[k] = k < K ? win[k] : 0.0;
  const auto kern = K == kQCommonK ? pair_quality_k<U8, kQCommonK> : pair_quality_k<U8, 0>;
  hipLaunchKernelGGL(kern, dim3((unsigned)planes), dim3(kQThreads), 0, st, a, b, C, H, W, qw, K, c1, c2, region, (int)(region_rows == 1), out,
                     ssim_map);
  return check_launch(name);
}

extern "C" {

int afd_pair_quality_f32(const float* a, const float* b, long planes, int C, int H, int W, const double* win, int K, double c1, double c2,
                         const uint8_t* region, long region_rows, double* out, double* ssim_map, afd_stream_t st) {
  return launch_pair_quality<false>("afd_pair_quality_f32", a, b, planes, C, H, W, win, K, c1, c2, region, region_rows, out, ssim_map, as_stream(st));
}

int afd_pair_quality_u8(const uint8_t* a, const uint8_t* b, long planes, int C, int H, int W, const double* win, int K, double c1, double c2,
                        const uint8_t* region, long region_rows, double* out, double* ssim_map, afd_stream_t st) {
  return launch_pair_quality<true>("afd_pair_quality_u8", a, b, planes, C, H, W, win, K, c1, c2, region, region_rows, out, ssim_map, as_stream(st));
}

}  // extern "C"

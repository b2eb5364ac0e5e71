// spectrum.hip -- mean power spectrum of a set of images, in fp64: power[c][u][v] = (1 / n) sum_i |F_{i,c}[u][v]|^2 with F the 2-D DFT
// (numpy's convention, rfft2 layout) of plane (i, c) after the optional mean removal and window, and its weighted radial sums.
// DESIGN.md section 6p has the semantics, the error budget and the cost.
//
// A plane is at most 64 x 64, so its DFT is two small matrix products on the fp64 matrix pipe (mfma_f64_16x16x4_f64):
//   pass 1   Y = X T_W        T_W = [cos | -sin](2 pi x v / W), v < Wh = W / 2 + 1          (H x W) (W x 2 Wh)
//   pass 2   Fr = C_H Yr + S_H Yi,  Fi = C_H Yi - S_H Yr     C_H / S_H = cos / sin(2 pi u y / H)      (H x 2 H) (2 H x Wh)
// The twiddles are never stored as matrices: a workgroup holds cos and sin of 2 pi m / N for m < N (N = W and N = H) and a lane
// looks its operand up at (j k) mod N, an integer it carries from K step to K step.  Sizes that are no multiple of the tile are
// zeros in the OPERANDS (a masked load), never in the accumulators.
// Workgroup (g, c) walks channel c of the images of slice g, keeps sum |F|^2 in registers and leaves one (H, Wh) partial in the
// workspace; spectrum_finish_k folds the partials in a fixed tree, divides by n once and reduces the radial sums in a fixed order.
// No atomics, no memset, nothing depends on the order in which workgroups run: the same arguments give the same bits.
#include "f64_tile.h"                              // v4d, mma_f64 and the fragment layout; the tiles here are a shape of their own

namespace afd {

constexpr int kSpMax = 64;                         // largest H and W
constexpr int kSpThreads = 256;                    // 4 waves; the 4 x 3 tiles of a 64 x 33 result are 3 per wave
constexpr int kSpTiles = 3;
constexpr int kSpPer = kSpMax * kSpMax / kSpThreads;      // elements of a plane per thread
constexpr int kXPitch = 68;                        // X[y][x]: 16 rows x 4 k per A fragment, rows 8 banks apart
constexpr int kYPitch = 48;                        // Y[y][v]: 4 k x 16 columns per B fragment, rows 32 banks apart
constexpr int kYImag = kSpMax * kYPitch;           // Yi behind Yr
constexpr int kSpBuf = 2 * kSpMax * kYPitch;       // X and Y share one buffer (Y waits in registers until X is no longer read)
static_assert(kSpBuf >= kSpMax * kXPitch && kSpMax / 2 + 1 <= kYPitch && kSpTiles * 4 >= (kSpMax / 16) * ((kSpMax / 2 + 1 + 15) / 16),
              "the buffer holds X, the tiles cover the result");
constexpr long kSpTarget = 768;                    // workgroups of a launch, whatever the device (three fit one of 256 CUs)

// cos and sin of 2 pi m / N for 0 <= m < N.  The quadrant and the remainder are integers, so sincospi sees an argument in [0, 1/2)
// that is one rounding away from exact, and the multiples of a quarter turn come out as exact 0 and +-1.
__device__ __forceinline__ void unit_root(int m, int N, double& c, double& s) {
  const int q = 4 * m / N, rem = 4 * m - q * N;
  double sr, cr;
  sincospi(0.5 * (double)rem / (double)N, &sr, &cr);
  c = q == 0 ? cr : q == 1 ? -sr : q == 2 ? -cr : sr;
  s = q == 0 ? sr : q == 1 ? cr : q == 2 ? -sr : -cr;
}

template <bool U8>
__global__ __launch_bounds__(kSpThreads, 3) void spectrum_k(const void* __restrict__ images, const float* __restrict__ table, long n, int C, int H,
                                                         int W, const double* __restrict__ win_h, const double* __restrict__ win_w,
                                                         int remove_mean, long per, long G, double* __restrict__ ws) {
  __shared__ double buf[kSpBuf];
  __shared__ double cw[kSpMax], sw[kSpMax], ch[kSpMax], sh[kSpMax], wh[kSpMax], ww[kSpMax];
  __shared__ double red[kSpThreads / kWave];
  const int tid = threadIdx.x, lane = tid & 63, c16 = lane & 15, g4 = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);      // scalar: the branches around the MFMAs are taken by whole waves
  const long g = blockIdx.x / C;
  const int c = (int)(blockIdx.x - g * C);
  const int Wh = W / 2 + 1, HW = H * W, NT = (Wh + 15) >> 4, ntiles = ((H + 15) >> 4) * NT, K1 = (W + 3) >> 2, K2 = (H + 3) >> 2;
  if (tid < W) {
    unit_root(tid, W, cw[tid], sw[tid]);
    ww[tid] = win_w ? win_w[tid] : 1.0;
  }
  if (tid >= kSpMax && tid - kSpMax < H) {
    const int m = tid - kSpMax;
    unit_root(m, H, ch[m], sh[m]);
    wh[m] = win_h ? win_h[m] : 1.0;
  }
  __syncthreads();
  // where this thread's elements of a plane go in X, y << 8 | x: the same for every plane
  int at[kSpPer];
#pragma unroll
  for (int j = 0; j < kSpPer; ++j) {
    const int e = tid + kSpThreads * j, y = e / W, x = e - y * W;
    at[j] = e < HW ? (y << 8 | x) : -1;
  }
  v4d acc[kSpTiles];
#pragma unroll
  for (int i = 0; i < kSpTiles; ++i) acc[i] = v4d{0.0, 0.0, 0.0, 0.0};

  const long i_end = (g + 1) * per < n ? (g + 1) * per : n;
  for (long img = g * per; img < i_end; ++img) {
    const long base = (img * C + c) * (long)HW;
    double v[kSpPer];
#pragma unroll
    for (int j = 0; j < kSpPer; ++j) {
      v[j] = 0.0;
      if (at[j] >= 0) {
        const long e = base + tid + kSpThreads * j;
        v[j] = U8 ? (double)table[(long)c * 256 + static_cast<const uint8_t*>(images)[e]] : (double)static_cast<const float*>(images)[e];
      }
    }
    double mean = 0.0;
    if (remove_mean) {                               // (uniform) the plane's sum in a fixed order: lanes' own sums, a shuffle tree, the waves
      double s = 0.0;
#pragma unroll
      for (int j = 0; j < kSpPer; ++j) s += v[j];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, kWave);
      if (lane == 0) red[w] = s;
      __syncthreads();
      mean = (((red[0] + red[1]) + red[2]) + red[3]) / (double)HW;
    }
#pragma unroll
    for (int j = 0; j < kSpPer; ++j)
      if (at[j] >= 0) buf[(at[j] >> 8) * kXPitch + (at[j] & 255)] = (v[j] - mean) * (wh[at[j] >> 8] * ww[at[j] & 255]);
    __syncthreads();

    // pass 1: tile (mt, nt) of Yr and Yi, K = x
    v4d yr[kSpTiles], yi[kSpTiles];
#pragma unroll
    for (int i = 0; i < kSpTiles; ++i) {
      yr[i] = yi[i] = v4d{0.0, 0.0, 0.0, 0.0};
      const int t = w + 4 * i;
      if (t < ntiles) {
        const int mt = t / NT, nt = t - mt * NT, row = 16 * mt + c16, vc = 16 * nt + c16;
        const bool rok = row < H, vok = vc < Wh;
        int idx = (g4 * vc) % W;
        const int step = (4 * vc) % W;
        for (int kk = 0; kk < K1; ++kk) {
          const int k = 4 * kk + g4;
          const double a = (rok && k < W) ? buf[row * kXPitch + k] : 0.0;
          const double br = vok ? cw[idx] : 0.0, bi = vok ? -sw[idx] : 0.0;
          yr[i] = mma_f64(a, br, yr[i]);
          yi[i] = mma_f64(a, bi, yi[i]);
          idx += step;
          idx -= idx >= W ? W : 0;
        }
      }
    }
    __syncthreads();                                 // X is no longer read: Y goes over it
#pragma unroll
    for (int i = 0; i < kSpTiles; ++i) {
      const int t = w + 4 * i;
      if (t < ntiles) {
        const int mt = t / NT, nt = t - mt * NT;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int o = (16 * mt + g4 + 4 * r) * kYPitch + 16 * nt + c16;
          buf[o] = yr[i][r];
          buf[kYImag + o] = yi[i][r];
        }
      }
    }
    __syncthreads();

    // pass 2: tile (ut, nt) of Fr and Fi, K = y.  Rows y >= H of Y are exact zeros (they came from masked rows of X).
#pragma unroll
    for (int i = 0; i < kSpTiles; ++i) {
      const int t = w + 4 * i;
      if (t < ntiles) {
        const int ut = t / NT, nt = t - ut * NT, u = 16 * ut + c16, vc = 16 * nt + c16;
        int idx = (g4 * u) % H;
        const int step = (4 * u) % H;
        v4d fr = v4d{0.0, 0.0, 0.0, 0.0}, fi = fr;
        for (int kk = 0; kk < K2; ++kk) {
          const int o = (4 * kk + g4) * kYPitch + vc;
          const double cc = ch[idx], ss = sh[idx], br = buf[o], bi = buf[kYImag + o];
          fr = mma_f64(cc, br, fr);
          fi = mma_f64(cc, bi, fi);
          fr = mma_f64(ss, bi, fr);
          fi = mma_f64(-ss, br, fi);
          idx += step;
          idx -= idx >= H ? H : 0;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[i][r] += fr[r] * fr[r] + fi[r] * fi[r];
      }
    }
    __syncthreads();                                 // Y is no longer read: the next plane goes over it
  }

  double* out = ws + (long)c * (H * Wh) * G + g;      // ws[c][u][v][slice]
#pragma unroll
  for (int i = 0; i < kSpTiles; ++i) {
    const int t = w + 4 * i;
    if (t < ntiles) {
      const int ut = t / NT, nt = t - ut * NT, vc = 16 * nt + c16;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int u = 16 * ut + g4 + 4 * r;
        if (u < H && vc < Wh) out[(long)(u * Wh + vc) * G] = acc[i][r];
      }
    }
  }
}

// The partials lie as ws[c][u][v][g], the slices of one coefficient side by side.  Workgroup (c, b) finishes the coefficients of
// one group b: with a bin map, group b < R is bin b and groups R .. R + kSpLeftOut - 1 share the coefficients that no bin takes
// (launched only when power is wanted); without one, group b is coefficients 16 b .. 16 b + 15.  A wave takes 64 coefficients at a
// time, finds its group's among them with one ballot and walks them in index order; per coefficient the lanes sum the slices
// g = lane, lane + 64, ..., a shuffle tree adds the lanes, and the sum is divided by n once.  radial[c][b] = the waves' sums of
// m(v) power, each in index order, added in wave order; m(v) = 1 on the columns that are their own mirror image (v = 0, and
// v = W / 2 for an even W), 2 elsewhere.  The bits of an output do not depend on whether the other one is asked for.
constexpr int kSpLeftOut = 8;

__global__ __launch_bounds__(kSpThreads) void spectrum_finish_k(const double* __restrict__ ws, long G, long n, int H, int W,
                                                                const int* __restrict__ bins, long R, long NB, double* __restrict__ power,
                                                                double* __restrict__ radial) {
  __shared__ double red[kSpThreads / kWave];
  const int lane = threadIdx.x & 63, Wh = W / 2 + 1, HWh = H * Wh;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long c = blockIdx.x / NB, b = blockIdx.x - c * NB;
  double acc = 0.0;                                  // lane 0: this wave's share of radial[c][b]
  for (int e0 = kWave * w; e0 < HWh; e0 += kSpThreads) {
    const int e = e0 + lane;
    bool mine = false;
    if (e < HWh) {
      if (bins) {
        const long q = bins[e];
        mine = b < R ? q == b : ((q < 0 || q >= R) && (e >> 4) % kSpLeftOut == b - R);
      } else {
        mine = (e >> 4) == b;
      }
    }
    unsigned long long todo = __ballot(mine);
    while (todo) {
      const int ee = e0 + __ffsll(todo) - 1;
      todo &= todo - 1;
      const double* p = ws + (c * HWh + ee) * G;
      double s = 0.0;
#pragma unroll 4
      for (long g = lane; g < G; g += kWave) s += p[g];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, kWave);
      if (lane == 0) {
        s = s / (double)n;
        if (power) power[c * HWh + ee] = s;
        const int v = ee % Wh;
        acc += (v == 0 || 2 * v == W) ? s : 2.0 * s;
      }
    }
  }
  if (!radial || b >= R) return;
  if (lane == 0) red[w] = acc;
  __syncthreads();
  if (threadIdx.x == 0) radial[c * R + b] = ((red[0] + red[1]) + red[2]) + red[3];
}

static bool sp_sizes_ok(long n, long C, long H, long W) {
  return n > 0 && C > 0 && H >= 1 && H <= kSpMax && W >= 1 && W <= kSpMax && n < (1L << 31) && C < (1L << 31) && C <= (1L << 40) / n;
}
// the most slices a call uses: the workspace is sized by it, the launch may use fewer (no slice is empty)
static long sp_slices(long n, long C) {
  const long t = kSpTarget / C > 1 ? kSpTarget / C : 1;
  return n < t ? n : t;
}

}  // namespace afd
using namespace afd;

template <bool U8>
static int launch_spectrum(const char* name, const void* images, const float* table, long n, long C, long H, long W, const double* win_h,
                           const double* win_w, int remove_mean, const int* bins, long R, double* power, double* radial, void* workspace,
                           size_t workspace_bytes, hipStream_t st) {
  AFD_REQUIRE(images, "%s: images must not be NULL", name);
  AFD_REQUIRE(!U8 || table, "%s: table must not be NULL", name);
  AFD_REQUIRE(workspace, "%s: workspace must not be NULL", name);
  AFD_REQUIRE(power || radial, "%s: power and radial must not both be NULL", name);
  AFD_REQUIRE(!radial || bins, "%s: bins must not be NULL when radial is given", name);
  AFD_REQUIRE(!radial || R > 0, "%s: R must be positive when radial is given (got %ld)", name, R);
  AFD_REQUIRE(n > 0 && C > 0, "%s: n and C must be positive (got %ld, %ld)", name, n, C);
  AFD_REQUIRE(H >= 1 && H <= kSpMax && W >= 1 && W <= kSpMax, "%s: H and W must lie in [1, %d] (got %ld, %ld)", name, kSpMax, H, W);
  AFD_REQUIRE(n < (1L << 31), "%s: n must be below 2^31 (got %ld)", name, n);
  AFD_REQUIRE(sp_sizes_ok(n, C, H, W), "%s: C must be below 2^31 and n C at most 2^40 (got n = %ld, C = %ld)", name, n, C);
  if (!radial) {
    bins = nullptr;
    R = 0;
  }
  AFD_REQUIRE(R + kSpLeftOut <= ((1L << 31) - 1) / C, "%s: C (R + %d) must be below 2^31 (got C = %ld, R = %ld)", name, kSpLeftOut, C, R);
  struct { const void* p; const char* what; } a8[] = {{power, "power"}, {radial, "radial"}, {win_h, "win_h"}, {win_w, "win_w"},
                                                      {workspace, "workspace"}};
  for (const auto& a : a8) AFD_REQUIRE(((uintptr_t)a.p & 7) == 0, "%s: %s must be 8-byte aligned", name, a.what);
  AFD_REQUIRE(((uintptr_t)bins & 3) == 0, "%s: bins must be 4-byte aligned", name);
  AFD_REQUIRE(((uintptr_t)table & 3) == 0, "%s: table must be 4-byte aligned", name);
  AFD_REQUIRE(U8 || ((uintptr_t)images & 3) == 0, "%s: images must be 4-byte aligned", name);
  const size_t need = afd_spectrum_workspace_bytes(n, C, H, W);
  AFD_REQUIRE(workspace_bytes >= need, "%s: workspace too small: %zu bytes given, afd_spectrum_workspace_bytes asks for %zu", name,
              workspace_bytes, need);
  const long Wh = W / 2 + 1, pb = C * H * Wh * 8, rb = C * R * 8;
  struct { const void* p; long bytes; const char* what; } in[] = {{images, n * C * H * W * (U8 ? 1 : 4), "images"},
                                                                  {U8 ? table : nullptr, C * 256 * 4, "table"},
                                                                  {win_h, H * 8, "win_h"},
                                                                  {win_w, W * 8, "win_w"},
                                                                  {bins, H * Wh * 4, "bins"}};
  for (const auto& a : in)
    AFD_REQUIRE(!(power && overlaps(power, pb, a.p, a.bytes)) && !(radial && overlaps(radial, rb, a.p, a.bytes)) &&
                    !overlaps(workspace, (long)need, a.p, a.bytes),
                "%s: power, radial and workspace must not overlap %s", name, a.what);
  AFD_REQUIRE(!(power && overlaps(power, pb, radial, rb)) && !overlaps(workspace, (long)need, power, pb) &&
                  !overlaps(workspace, (long)need, radial, rb),
              "%s: power, radial and workspace must not overlap each other", name);
  const long per = (n + sp_slices(n, C) - 1) / sp_slices(n, C), G = (n + per - 1) / per;
  double* ws = static_cast<double*>(workspace);
  hipLaunchKernelGGL(spectrum_k<U8>, dim3((unsigned)(G * C)), dim3(kSpThreads), 0, st, images, table, n, (int)C, (int)H, (int)W, win_h, win_w,
                     remove_mean, per, G, ws);
  const long NB = radial ? R + (power ? kSpLeftOut : 0) : (H * Wh + 15) / 16;
  hipLaunchKernelGGL(spectrum_finish_k, dim3((unsigned)(C * NB)), dim3(kSpThreads), 0, st, ws, G, n, (int)H, (int)W, bins, R, NB, power, radial);
  return check_launch(name);
}

extern "C" {

size_t afd_spectrum_workspace_bytes(long n, long C, long H, long W) {
  if (!sp_sizes_ok(n, C, H, W)) return 0;
  return (size_t)sp_slices(n, C) * (size_t)C * (size_t)H * (size_t)(W / 2 + 1) * sizeof(double);
}

int afd_power_spectrum_u8(const uint8_t* images, const float* table, long n, long C, long H, long W, const double* win_h, const double* win_w,
                          int remove_mean, const int* bins, long R, double* power, double* radial, void* workspace, size_t workspace_bytes,
                          afd_stream_t st) {
  return launch_spectrum<true>("afd_power_spectrum_u8", images, table, n, C, H, W, win_h, win_w, remove_mean, bins, R, power, radial, workspace,
                               workspace_bytes, as_stream(st));
}

int afd_power_spectrum_f32(const float* images, long n, long C, long H, long W, const double* win_h, const double* win_w, int remove_mean,
                           const int* bins, long R, double* power, double* radial, void* workspace, size_t workspace_bytes, afd_stream_t st) {
  return launch_spectrum<false>("afd_power_spectrum_f32", images, nullptr, n, C, H, W, win_h, win_w, remove_mean, bins, R, power, radial,
                                workspace, workspace_bytes, as_stream(st));
}

}  // extern "C"

// rotate.hip -- F17 (Config E): scipy.ndimage.rotate(x, angle, axes=(2,3), reshape=False, order=3,
// mode='grid-wrap', prefilter=True) on the device, replacing the reference's per-step
// D2H -> CPU spline -> H2D round trip (ddpm_models.py:421-429).
//
// scipy works plane by plane in float64: (1) cubic B-spline prefilter along axis 0 then axis 1 -- gain
// (1-z)(1-1/z) = 6, pole z = sqrt(3)-2, periodic ('grid-wrap') initial conditions, causal then
// anti-causal recursion; (2) for every output pixel the input coordinate  M (o) + offset  is mapped
// into the period, the 4x4 footprint starts at floor(c)-1, indices wrap, weights are the cubic
// B-spline pieces.  The recursions and weight formulas below restate that arithmetic in the same
// order and precision (fp64); the result is rounded once to fp32 like scipy's float32 output array.
#include "common.h"

namespace afd {

constexpr double kPole = -0.26794919243112270647;      // sqrt(3) - 2

// one thread per line; `stride` = element distance along the filtered axis, lines are `lstride` apart
__global__ __launch_bounds__(128) void spline3_prefilter_wrap(double* __restrict__ c, int n, long stride, long lines,
                                                              int inner, long lstride_outer, long lstride_inner) {
  const long ln = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (ln >= lines) return;
  double* p = c + (ln / inner) * lstride_outer + (ln % inner) * lstride_inner;
  const double z = kPole;
  if (n < 2) return;
  const double gain = (1.0 - z) * (1.0 - 1.0 / z);
  for (int i = 0; i < n; ++i) p[i * stride] *= gain;
  // causal initialisation (periodic): c[0] += sum_{i=1}^{n-1} z^i c[n-i];  c[0] /= 1 - z^n
  double zi = z, c0 = p[0];
  for (int i = 1; i < n; ++i) { c0 += zi * p[(long)(n - i) * stride]; zi *= z; }
  p[0] = c0 / (1.0 - zi);
  for (int i = 1; i < n; ++i) p[i * stride] += z * p[(i - 1) * stride];
  // anti-causal initialisation: c[n-1] += sum_{i=0}^{n-2} z^(i+1) c[i];  c[n-1] *= z / (z^n - 1)
  zi = z; double cl = p[(long)(n - 1) * stride];
  for (int i = 0; i < n - 1; ++i) { cl += zi * p[i * stride]; zi *= z; }
  p[(long)(n - 1) * stride] = cl * (z / (zi - 1.0));
  for (int i = n - 2; i >= 0; --i) p[i * stride] = z * (p[(i + 1) * stride] - p[i * stride]);
}

__global__ void f32_to_f64(const float* __restrict__ x, double* __restrict__ y, long n) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) y[i] = (double)x[i];
}

__device__ __forceinline__ double map_grid_wrap(double in, int len) {
  if (len <= 1) return 0.0;
  if (in < 0) in += (double)len * (double)((long)((-1.0 - in) / len) + 1);
  else if (in > len - 1) { in -= (double)len * (double)((long)((in + 1.0) / len)); if (in < 0) in += len; }
  return in;
}
__device__ __forceinline__ void spline3_weights(double x, double (&w)[4]) {
  x -= floor(x);
  const double y = x, z = 1.0 - x;
  w[1] = (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0;
  w[2] = (z * z * (z - 2.0) * 3.0 + 4.0) / 6.0;
  w[0] = z * z * z / 6.0;
  w[3] = 1.0 - w[0] - w[1] - w[2];
}
__device__ __forceinline__ int wrap_idx(int i, int n) { i %= n; return i < 0 ? i + n : i; }

// One output pixel in fp64: sum_{i,j} cp[wrap(sy+i), wrap(sx+j)] * wy[i] * wx[j] at the wrapped source coordinate of (oy, ox).
// Every kernel below evaluates the spline through this one function, so they agree bit for bit.
__device__ __forceinline__ double spline3_at(const double* __restrict__ cp, int H, int W, int oy, int ox, double m00, double m01,
                                             double m10, double m11, double off0, double off1) {
  double cy = m00 * oy + m01 * ox + off0;
  double cx = m10 * oy + m11 * ox + off1;
  cy = map_grid_wrap(cy, H); cx = map_grid_wrap(cx, W);
  double wy[4], wx[4];
  spline3_weights(cy, wy); spline3_weights(cx, wx);
  const int sy = (int)floor(cy) - 1, sx = (int)floor(cx) - 1;
  double t = 0.0;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int yy = wrap_idx(sy + a, H);
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      double v = cp[(long)yy * W + wrap_idx(sx + b, W)];
      v *= wy[a]; v *= wx[b];
      t += v;
    }
  }
  return t;
}

// out[p, oy, ox] = the spline of plane p at M (oy, ox) + off, rounded once to fp32
__global__ void spline3_affine_wrap(const double* __restrict__ coef, float* __restrict__ out, long planes, int H, int W,
                                    double m00, double m01, double m10, double m11, double off0, double off1) {
  const long total = planes * H * W;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int ox = i % W, oy = (i / W) % H; const long p = i / ((long)W * H);
    out[i] = (float)spline3_at(coef + p * (long)H * W, H, W, oy, ox, m00, m01, m10, m11, off0, off1);
  }
}

// Row r of out (C planes) = source field img[r] of coef (n_src fields of C planes) resampled by transform k[r] of the (K, 6)
// table affine = [m00, m01, m10, m11, off0, off1]: spline3_affine_wrap's value of that field under that transform, bit for bit.
__global__ void spline3_affine_wrap_rows(const double* __restrict__ coef, const int64_t* __restrict__ img,
                                         const double* __restrict__ affine, const int64_t* __restrict__ k,
                                         float* __restrict__ out, long rows, int C, int H, int W) {
  const long hw = (long)H * W, per = C * hw, total = rows * per;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long r = i / per, e = i % per;
    const int ox = e % W, oy = (e / W) % H; const long c = e / hw;
    const double* a = affine + 6 * k[r];
    out[i] = (float)spline3_at(coef + (img[r] * C + c) * hw, H, W, oy, ox, a[0], a[1], a[2], a[3], a[4], a[5]);
  }
}

// The validity mask of a transform at output pixel (oy, ox) for margin m: the pixel and its unwrapped source M o + off both lie
// in [m, H-1-m] x [m, W-1-m].  Two products and two sums per coordinate, each rounded (no fused multiply-add), so that the
// host's numpy statement of the mask (Diffusion.equivariance_mask) decides boundary pixels the same way.
__device__ __forceinline__ bool eq_mask_at(int H, int W, int oy, int ox, const double* a, double m) {
#pragma clang fp contract(off)
  const double py = a[0] * oy, qy = a[1] * ox, px = a[2] * oy, qx = a[3] * ox;
  const double cy = (py + qy) + a[4], cx = (px + qx) + a[5];
  const double hy = (double)(H - 1) - m, hx = (double)(W - 1) - m;
  return oy >= m && oy <= hy && ox >= m && ox <= hx && cy >= m && cy <= hy && cx >= m && cx <= hx;
}

// Sum of three fp64 values over a 256-thread workgroup in a fixed order: a shuffle tree inside each wave, then the four waves'
// partial sums in wave order.  The result is valid in thread 0.  red: 12 doubles of LDS.
__device__ __forceinline__ void block_sum3_f64(double& a, double& b, double& c, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_down(a, o, kWave);
    b += __shfl_down(b, o, kWave);
    c += __shfl_down(c, o, kWave);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[3 * w] = a; red[3 * w + 1] = b; red[3 * w + 2] = c; }
  __syncthreads();
  if (threadIdx.x == 0) {
    a = red[0]; b = red[1]; c = red[2];
    for (int i = 1; i < (int)(blockDim.x >> 6); ++i) { a += red[3 * i]; b += red[3 * i + 1]; c += red[3 * i + 2]; }
  }
}

// Equivariance terms, one workgroup per row.  With ref = the spline of source field img[r] under transform k[r] in fp64 (never
// rounded, never stored) and d = double(g) - ref over the masked pixels of all C planes:
//   out[r] = [sum d^2, sum ref^2, number of masked elements (masked pixels * C)]
// Thread i takes elements i, i + 256, ... in that order; pixels outside the mask are skipped before any coefficient is read.
__global__ __launch_bounds__(256) void eq_terms_k(const double* __restrict__ coef, const int64_t* __restrict__ img,
                                                  const double* __restrict__ affine, const int64_t* __restrict__ k,
                                                  const float* __restrict__ g, double margin, double* __restrict__ out,
                                                  int C, int H, int W) {
  __shared__ double red[12];
  const long r = blockIdx.x, hw = (long)H * W, per = C * hw;
  const double* a = affine + 6 * k[r];
  const double* src = coef + img[r] * per;
  const float* gr = g + r * per;
  const double m00 = a[0], m01 = a[1], m10 = a[2], m11 = a[3], off0 = a[4], off1 = a[5];
  double s_d = 0.0, s_r = 0.0, cnt = 0.0;
  for (long e = threadIdx.x; e < per; e += blockDim.x) {
    const int ox = e % W, oy = (e / W) % H; const long c = e / hw;
    if (!eq_mask_at(H, W, oy, ox, a, margin)) continue;
    const double ref = spline3_at(src + c * hw, H, W, oy, ox, m00, m01, m10, m11, off0, off1);
    const double d = (double)gr[e] - ref;
    s_d += d * d;
    s_r += ref * ref;
    cnt += 1.0;
  }
  block_sum3_f64(s_d, s_r, cnt, red);
  if (threadIdx.x == 0) { out[3 * r] = s_d; out[3 * r + 1] = s_r; out[3 * r + 2] = cnt; }
}

}  // namespace afd
using namespace afd;

extern "C" {

size_t afd_rotate_workspace_bytes(long planes, int H, int W) { return sizeof(double) * (size_t)planes * H * W; }

// x (planes, H, W) fp32 -> its cubic B-spline coefficients in fp64: the conversion and the two recursive passes
int afd_spline3_prefilter_wrap(const float* x, double* coef, long planes, int H, int W, afd_stream_t st) {
  AFD_REQUIRE(x && coef, "afd_spline3_prefilter_wrap: x and coef must not be NULL");
  AFD_REQUIRE(planes > 0 && H > 0 && W > 0, "afd_spline3_prefilter_wrap: planes, H and W must be positive (got %ld, %d, %d)", planes, H, W);
  const long n = planes * H * W;
  AFD_REQUIRE(!overlaps(coef, n * (long)sizeof(double), x, n * (long)sizeof(float)), "afd_spline3_prefilter_wrap: coef must not overlap x");
  hipStream_t s = as_stream(st);
  long g = (n + 255) / 256; if (g > 32768) g = 32768;
  hipLaunchKernelGGL(f32_to_f64, dim3((unsigned)g), dim3(256), 0, s, x, coef, n);
  // axis 0 (rows direction): lines = (plane, column); then axis 1: lines = (plane, row)
  long lines = planes * W;
  hipLaunchKernelGGL(spline3_prefilter_wrap, dim3((unsigned)((lines + 127) / 128)), dim3(128), 0, s, coef, H, (long)W, lines, W, (long)H * W, 1L);
  lines = planes * H;
  hipLaunchKernelGGL(spline3_prefilter_wrap, dim3((unsigned)((lines + 127) / 128)), dim3(128), 0, s, coef, W, 1L, lines, H, (long)H * W, (long)W);
  return check_launch("afd_spline3_prefilter_wrap");
}

// matrix / offset are the affine map scipy builds for `rotate`: in = M @ out + offset (row, col order)
int afd_affine_spline3_wrap(const float* x, float* y, long planes, int H, int W, const double* matrix4, const double* offset2,
                            void* workspace, afd_stream_t st) {
  AFD_REQUIRE(x && y && matrix4 && offset2 && workspace && planes > 0 && H > 0 && W > 0, "afd_affine_spline3_wrap: bad argument");
  double* c = static_cast<double*>(workspace);
  if (int rc = afd_spline3_prefilter_wrap(x, c, planes, H, W, st)) return rc;
  const long n = planes * H * W;
  long g = (n + 255) / 256; if (g > 32768) g = 32768;
  hipLaunchKernelGGL(spline3_affine_wrap, dim3((unsigned)g), dim3(256), 0, as_stream(st), c, y, planes, H, W,
                     matrix4[0], matrix4[1], matrix4[2], matrix4[3], offset2[0], offset2[1]);
  return check_launch("afd_affine_spline3_wrap");
}

#define AFD_ROWS_CHECKS(name)                                                                                                \
  AFD_REQUIRE(coef && img && affine && k, name ": no pointer may be NULL");                                                   \
  AFD_REQUIRE(n_src > 0 && K > 0 && rows > 0 && C > 0 && H > 0 && W > 0,                                                      \
              name ": n_src, K, rows, C, H and W must be positive (got %ld, %ld, %ld, %d, %d, %d)", n_src, K, rows, C, H, W); \
  AFD_REQUIRE(rows <= 0x7fffffffL, name ": at most 2^31 - 1 rows per call (got %ld)", rows)

int afd_affine_spline3_wrap_rows(const double* coef, long n_src, const int64_t* img, const double* affine, long K, const int64_t* k,
                                 float* out, long rows, int C, int H, int W, afd_stream_t st) {
  AFD_REQUIRE(out, "afd_affine_spline3_wrap_rows: no pointer may be NULL");
  AFD_ROWS_CHECKS("afd_affine_spline3_wrap_rows");
  const long per = (long)C * H * W, ob = rows * per * (long)sizeof(float), ib = rows * (long)sizeof(int64_t);
  AFD_REQUIRE(!overlaps(out, ob, coef, n_src * per * (long)sizeof(double)) && !overlaps(out, ob, img, ib) && !overlaps(out, ob, k, ib) &&
                  !overlaps(out, ob, affine, 6 * K * (long)sizeof(double)),
              "afd_affine_spline3_wrap_rows: out must not overlap any input");
  const long n = rows * per;
  long g = (n + 255) / 256; if (g > 32768) g = 32768;
  hipLaunchKernelGGL(spline3_affine_wrap_rows, dim3((unsigned)g), dim3(256), 0, as_stream(st), coef, img, affine, k, out, rows, C, H, W);
  return check_launch("afd_affine_spline3_wrap_rows");
}

int afd_eq_terms(const double* coef, long n_src, const int64_t* img, const double* affine, long K, const int64_t* k, const float* g,
                 double margin, double* out, long rows, int C, int H, int W, afd_stream_t st) {
  AFD_REQUIRE(g && out, "afd_eq_terms: no pointer may be NULL");
  AFD_ROWS_CHECKS("afd_eq_terms");
  AFD_REQUIRE(margin >= 0.0 && margin < 1e300, "afd_eq_terms: margin must be finite and >= 0 (got %g)", margin);
  const long per = (long)C * H * W, ob = 3 * rows * (long)sizeof(double), ib = rows * (long)sizeof(int64_t);
  AFD_REQUIRE(!overlaps(out, ob, coef, n_src * per * (long)sizeof(double)) && !overlaps(out, ob, img, ib) && !overlaps(out, ob, k, ib) &&
                  !overlaps(out, ob, affine, 6 * K * (long)sizeof(double)) && !overlaps(out, ob, g, rows * per * (long)sizeof(float)),
              "afd_eq_terms: out must not overlap any input");
  hipLaunchKernelGGL(eq_terms_k, dim3((unsigned)rows), dim3(256), 0, as_stream(st), coef, img, affine, k, g, margin, out, C, H, W);
  return check_launch("afd_eq_terms");
}

}  // extern "C"

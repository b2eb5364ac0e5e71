// posterior.hip -- diffusion posterior sampling (DPS, Chung et al. 2023) for the linear operators A x = m . S_s(k * x): A, its
// adjoint, the fused residual-and-seed kernel of a sampling step, and the step's correction.
//
// k * x is a correlation with a K x K kernel (K odd, at most 15) and zero padding K / 2, S_s keeps every s-th row and column
// (s = 1, 2 or 4, the measurement plane is h x w = H / s x W / s) and m is a mask at measurement resolution: per channel
//   (A x)[i][j]   = m[i][j] sum_{a, b} k[a][b] x[i s - K/2 + a][j s - K/2 + b]                    (x is 0 outside the plane)
//   (A^T r)[p][q] = sum_{a, b} k[a][b] (m r)[(p + K/2 - a) / s][(q + K/2 - b) / s]               over the taps where both
//                                                                                                   divisions are exact and land in h x w
// One kernel template, one 256-thread workgroup per (row, channel) plane: the plane goes to LDS once (at most 64 x 64 floats, 16 KiB),
// every output element walks its window there with the taps (LDS too, read at one address by the whole wave: a broadcast), and the
// fused form keeps the masked residual in a second LDS plane for the adjoint, so x0_hat and r never reach memory.  With s = 1 a
// wave's 64 lanes read 64 consecutive floats per tap: no bank conflict.  With s = 2 (4) the lanes of the forward walk are 2 (4)
// floats apart, a 2-way (4-way) conflict on the 32 banks of ds_read_b32, on a plane with 4 (16) times fewer outputs.
// Tap sums: a outer, b inner, ascending, each step a fused multiply-add said as fmaf; everything else one IEEE rounding per
// operation (no contraction in this file).  A plane's sum of squares is taken in fp64: a thread adds its elements in index order, a
// shuffle tree adds the lanes, the four waves are added in order.  No atomics, no workspace: the same bits from call to call.
#include "common.h"

#pragma clang fp contract(off)

#include "diffusion_common.h"
#include "objective_common.h"

namespace afd {

constexpr int kLinMaxSide = 64;
constexpr int kLinThreads = 256;
constexpr int kLinPlane = kLinMaxSide * kLinMaxSide;

enum { kLinApply = 0, kLinAdjoint = 1, kLinResidual = 2 };

// x0_hat = a x_t + b out: (a, b) of `kind` at ah = alpha_hat[t], in fp64 from the fp32 table value and rounded once
struct DpsCoef {
  float a, b;
};
__device__ __forceinline__ DpsCoef dps_coef(int kind, float ah32) {
  const double ah = (double)ah32;
  const double sa = sqrt(ah), sb = sqrt(1.0 - ah);
  if (kind == AFD_PRED_V) return DpsCoef{(float)sa, (float)(-sb)};
  if (kind == AFD_PRED_X0) return DpsCoef{0.0f, 1.0f};
  return DpsCoef{(float)(1.0 / sa), (float)(-sb / sa)};
}

// post(o, acc) for every element o of the h x w plane S_s(k * src), src the H x W plane in LDS; only the taps inside the plane
// are visited (their bounds worked out up front, so the loops have no branch)
template <class Post>
__device__ __forceinline__ void linop_forward(const float* __restrict__ src, int H, int W, int h, int w, const float* __restrict__ taps,
                                              int K, int s, Post post) {
  const int pad = K >> 1;
  for (int o = threadIdx.x; o < h * w; o += kLinThreads) {
    const int i = o / w, j = o - i * w;
    const int p0 = i * s - pad, q0 = j * s - pad;                   // tap (a, b) reads src[p0 + a][q0 + b]
    const int a0 = max(0, -p0), a1 = min(K, H - p0), b0 = max(0, -q0), b1 = min(K, W - q0);
    float acc = 0.f;
    for (int a = a0; a < a1; ++a) {
      const float* __restrict__ kr = taps + a * K;
      const float* __restrict__ sr = src + (p0 + a) * W + q0;
      for (int b = b0; b < b1; ++b) acc = fmaf(kr[b], sr[b], acc);
    }
    post(o, acc);
  }
}

// dst (H x W, global) = the transposed strided correlation of src (h x w, LDS): tap (a, b) of output (p, q) reads
// src[(p + pad - a) / s][(q + pad - b) / s] where both are whole and inside, so a runs over a = (p + pad) mod s, + s, ...
__device__ __forceinline__ void linop_transposed(const float* __restrict__ src, float* __restrict__ dst, int H, int W, int h, int w,
                                                 const float* __restrict__ taps, int K, int s) {
  const int pad = K >> 1;
  for (int o = threadIdx.x; o < H * W; o += kLinThreads) {
    const int p = o / W, q = o - p * W;
    const int pp = p + pad, qq = q + pad;
    int a0 = max(0, pp - (h - 1) * s), b0 = max(0, qq - (w - 1) * s);
    a0 += (pp - a0) % s;                                            // the first a >= a0 with (pp - a) a multiple of s
    b0 += (qq - b0) % s;
    const int a1 = min(K - 1, pp), b1 = min(K - 1, qq);             // inclusive: (pp - a) / s >= 0
    float acc = 0.f;
    for (int a = a0; a <= a1; a += s) {
      const float* __restrict__ kr = taps + a * K;
      const float* __restrict__ sr = src + ((pp - a) / s) * w;
      for (int b = b0; b <= b1; b += s) acc = fmaf(kr[b], sr[(qq - b) / s], acc);
    }
    dst[o] = acc;
  }
}

struct LinOp {
  Taps taps;
  int K, s;
  const float* mask;          // (mask_channels, h, w) or NULL
  int mask_channels;          // 0 (no mask), 1 or C
};

// kLinApply:    in = x (planes, H, W),  out = y (planes, h, w)
// kLinAdjoint:  in = r (planes, h, w),  out = g (planes, H, W)
// kLinResidual: in = x_t, net = the network's output, y the measurement, out = g, sums[plane] = sum r^2
template <int MODE>
__global__ __launch_bounds__(kLinThreads) void linop_k(const float* __restrict__ in, const float* __restrict__ net,
                                                       const float* __restrict__ y, const int64_t* __restrict__ t_rows,
                                                       const float* __restrict__ alpha_hat, int kind, LinOp op, float* __restrict__ out,
                                                       double* __restrict__ sums, int C, int H, int W) {
  __shared__ float full[MODE == kLinAdjoint ? 1 : kLinPlane];       // the H x W plane
  __shared__ float meas[MODE == kLinApply ? 1 : kLinPlane];         // the h x w plane: m r
  __shared__ float taps[AFD_MAX_TAPS * AFD_MAX_TAPS];
  __shared__ double red[kLinThreads / kWave];
  const int tid = threadIdx.x, K = op.K, s = op.s;
  const long plane = blockIdx.x;
  const int h = H / s, w = W / s, HW = H * W, hw = h * w;
  for (int i = tid; i < K * K; i += kLinThreads) taps[i] = op.taps.k[i];      // (the first barrier below orders these writes)
  const float* m = op.mask ? op.mask + (long)(op.mask_channels == 1 ? 0 : plane % C) * hw : nullptr;

  if (MODE == kLinAdjoint) {
    const float* r = in + plane * hw;
    for (int o = tid; o < hw; o += kLinThreads) meas[o] = m ? m[o] * r[o] : r[o];
    __syncthreads();
    linop_transposed(meas, out + plane * HW, H, W, h, w, taps, K, s);
    return;
  }

  if (MODE == kLinApply) {
    const float* x = in + plane * HW;
    for (int e = tid; e < HW; e += kLinThreads) full[e] = x[e];
    __syncthreads();
    float* yo = out + plane * hw;
    linop_forward(full, H, W, h, w, taps, K, s, [=](int o, float acc) { yo[o] = m ? m[o] * acc : acc; });
    return;
  }

  // the fused step side: x0_hat -> r -> (sum r^2, g)
  const DpsCoef ab = dps_coef(kind, alpha_hat[t_rows[plane / C]]);
  {
    const float *xt = in + plane * HW, *po = net + plane * HW;
    for (int e = tid; e < HW; e += kLinThreads) {
      const float l = ab.a * xt[e], r = ab.b * po[e];
      full[e] = l + r;
    }
  }
  __syncthreads();
  double sq = 0.0;
  {
    const float* yp = y + plane * hw;
    float* mr = meas;
    linop_forward(full, H, W, h, w, taps, K, s, [&](int o, float acc) {
      const float ax = m ? m[o] * acc : acc;
      const float r = ax - yp[o];
      sq += (double)r * (double)r;
      mr[o] = m ? m[o] * r : r;
    });
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sq += __shfl_down(sq, o, kWave);
  if ((tid & 63) == 0) red[tid >> 6] = sq;
  __syncthreads();                                                   // meas and red are complete
  if (tid == 0) {
    double tot = red[0];
#pragma unroll
    for (int k = 1; k < kLinThreads / kWave; ++k) tot += red[k];
    sums[plane] = tot;
  }
  linop_transposed(meas, out + plane * HW, H, W, h, w, taps, K, s);
}

// x[row] -= c_row (a_row g + b_row v), c_row = zeta / sqrt(sum_c sums[row][c]): `per_row` workgroups per row
__global__ __launch_bounds__(256) void dps_correct_k(float* x, const float* __restrict__ g, const float* __restrict__ v,
                                                     const double* __restrict__ sums, const int64_t* __restrict__ t_rows,
                                                     const float* __restrict__ alpha_hat, int kind, double zeta, int C, long chw,
                                                     int per_row) {
  const long row = blockIdx.x / per_row;
  const int part = blockIdx.x - (int)(row * per_row);
  double S = 0.0;
  for (int c = 0; c < C; ++c) S += sums[row * C + c];
  if (S == 0.0 || zeta == 0.0) return;                               // c_row = 0: the row stays as it is, bit for bit
  const float cr = (float)(zeta / sqrt(S));
  const DpsCoef ab = dps_coef(kind, alpha_hat[t_rows[row]]);
  const long base = row * chw;
  for (long e = (long)part * 256 + threadIdx.x; e < chw; e += (long)per_row * 256) {
    const float l = ab.a * g[base + e], r = ab.b * v[base + e];
    const float step = cr * (l + r);
    x[base + e] = x[base + e] - step;
  }
}

static int linop_args(const char* name, const float* kernel, int K, int stride, const float* mask, int mask_channels, long B, int C,
                      int H, int W, LinOp* op) {
  AFD_REQUIRE(B > 0 && C > 0 && B * C < (1L << 31), "%s: B and C must be positive with B C < 2^31 (got %ld, %d)", name, B, C);
  AFD_REQUIRE(K >= 1 && K <= AFD_MAX_TAPS && (K & 1), "%s: K must be odd and at most %d (got %d)", name, AFD_MAX_TAPS, K);
  AFD_REQUIRE(kernel || K == 1, "%s: kernel must not be NULL unless K == 1 (the delta)", name);
  AFD_REQUIRE(stride == 1 || stride == 2 || stride == 4, "%s: stride must be 1, 2 or 4 (got %d)", name, stride);
  AFD_REQUIRE(H >= 1 && W >= 1 && H <= kLinMaxSide && W <= kLinMaxSide && H % stride == 0 && W % stride == 0,
              "%s: H and W must lie in [1, %d] and be multiples of the stride (got %d, %d, stride %d)", name, kLinMaxSide, H, W, stride);
  AFD_REQUIRE(mask ? (mask_channels == 1 || mask_channels == C) : mask_channels == 0,
              "%s: mask_channels must be 1 or C with a mask and 0 without (got %d, C = %d)", name, mask_channels, C);
  op->K = K;
  op->s = stride;
  op->mask = mask;
  op->mask_channels = mask_channels;
  if (kernel)
    for (int i = 0; i < K * K; ++i) op->taps.k[i] = kernel[i];
  else
    op->taps.k[0] = 1.0f;
  return AFD_OK;
}

}  // namespace afd

using namespace afd;

extern "C" {

int afd_linop_apply(const float* x, float* y, const float* kernel, int K, int stride, const float* mask, int mask_channels, long B, int C,
                    int H, int W, afd_stream_t stream) {
  const char* name = "afd_linop_apply";
  AFD_REQUIRE(x && y, "%s: x and y must not be NULL", name);
  LinOp op;
  if (int rc = linop_args(name, kernel, K, stride, mask, mask_channels, B, C, H, W, &op)) return rc;
  const long planes = B * C, fb = planes * H * W * (long)sizeof(float), mb = fb / (stride * stride);
  AFD_REQUIRE(!overlaps(y, mb, x, fb) && !overlaps(y, mb, mask, (long)mask_channels * (mb / planes)), "%s: y must not overlap x or mask", name);
  hipLaunchKernelGGL(linop_k<kLinApply>, dim3((unsigned)planes), dim3(kLinThreads), 0, as_stream(stream), x, nullptr, nullptr, nullptr,
                     nullptr, 0, op, y, nullptr, C, H, W);
  return check_launch(name);
}

int afd_linop_adjoint(const float* r, float* g, const float* kernel, int K, int stride, const float* mask, int mask_channels, long B,
                      int C, int H, int W, afd_stream_t stream) {
  const char* name = "afd_linop_adjoint";
  AFD_REQUIRE(r && g, "%s: r and g must not be NULL", name);
  LinOp op;
  if (int rc = linop_args(name, kernel, K, stride, mask, mask_channels, B, C, H, W, &op)) return rc;
  const long planes = B * C, fb = planes * H * W * (long)sizeof(float), mb = fb / (stride * stride);
  AFD_REQUIRE(!overlaps(g, fb, r, mb) && !overlaps(g, fb, mask, (long)mask_channels * (mb / planes)), "%s: g must not overlap r or mask", name);
  hipLaunchKernelGGL(linop_k<kLinAdjoint>, dim3((unsigned)planes), dim3(kLinThreads), 0, as_stream(stream), r, nullptr, nullptr, nullptr,
                     nullptr, 0, op, g, nullptr, C, H, W);
  return check_launch(name);
}

int afd_dps_residual(const float* x_t, const float* out, const int64_t* t_rows, const float* alpha_hat, int prediction, const float* y,
                     const float* kernel, int K, int stride, const float* mask, int mask_channels, float* g, double* sums, long B, int C,
                     int H, int W, afd_stream_t stream) {
  const char* name = "afd_dps_residual";
  AFD_REQUIRE(x_t && out && t_rows && alpha_hat && y && g && sums, "%s: x_t, out, t_rows, alpha_hat, y, g and sums must not be NULL", name);
  AFD_REQUIRE_KIND(name, prediction);
  AFD_REQUIRE(((uintptr_t)sums & 7) == 0, "%s: sums must be 8-byte aligned", name);
  LinOp op;
  if (int rc = linop_args(name, kernel, K, stride, mask, mask_channels, B, C, H, W, &op)) return rc;
  const long planes = B * C, fb = planes * H * W * (long)sizeof(float), mb = fb / (stride * stride);
  const long sb = planes * (long)sizeof(double);
  AFD_REQUIRE(!overlaps(g, fb, x_t, fb) && !overlaps(g, fb, out, fb) && !overlaps(g, fb, y, mb) &&
                  !overlaps(g, fb, mask, (long)mask_channels * (mb / planes)) && !overlaps(g, fb, sums, sb) &&
                  !overlaps(sums, sb, x_t, fb) && !overlaps(sums, sb, out, fb) && !overlaps(sums, sb, y, mb) &&
                  !overlaps(sums, sb, mask, (long)mask_channels * (mb / planes)),
              "%s: g and sums must not overlap the inputs or each other", name);
  hipLaunchKernelGGL(linop_k<kLinResidual>, dim3((unsigned)planes), dim3(kLinThreads), 0, as_stream(stream), x_t, out, y, t_rows,
                     alpha_hat, prediction, op, g, sums, C, H, W);
  return check_launch(name);
}

int afd_dps_correct(float* x, const float* g, const float* v, const double* sums, const int64_t* t_rows, const float* alpha_hat,
                    int prediction, double zeta, long B, int C, long HW, afd_stream_t stream) {
  const char* name = "afd_dps_correct";
  AFD_REQUIRE(x && g && v && sums && t_rows && alpha_hat, "%s: x, g, v, sums, t_rows and alpha_hat must not be NULL", name);
  AFD_REQUIRE_KIND(name, prediction);
  AFD_REQUIRE(B > 0 && C > 0 && HW > 0 && B < (1L << 24), "%s: B, C and HW must be positive, B below 2^24 (got %ld, %d, %ld)", name, B, C, HW);
  AFD_REQUIRE(std::isfinite(zeta) && zeta >= 0.0, "%s: zeta must be finite and >= 0 (got %g)", name, zeta);
  const long chw = (long)C * HW, fb = B * chw * (long)sizeof(float);
  AFD_REQUIRE(!overlaps(x, fb, g, fb) && !overlaps(x, fb, v, fb) && !overlaps(x, fb, sums, B * C * (long)sizeof(double)),
              "%s: x must not overlap g, v or sums", name);
  const int per_row = (int)std::min<long>((chw + 255) / 256, 64);
  hipLaunchKernelGGL(dps_correct_k, dim3((unsigned)(B * per_row)), dim3(256), 0, as_stream(stream), x, g, v, sums, t_rows, alpha_hat,
                     prediction, zeta, C, chw, per_row);
  return check_launch(name);
}

}  // extern "C"

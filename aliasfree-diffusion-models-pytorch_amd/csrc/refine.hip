// refine.hip -- reference-guided sampling (ILVR, Choi et al. 2021): the low-pass refinement x <- x + phi(known - x) in one launch.
//
// phi_L(v) = 4^L U^L(D^L(v)) with D = the filtered 2x downsampler and U = the filtered 2x upsampler of filt.hip (cross-correlation,
// zero 'same' padding with lo = (N-1)/2, samples on even positions, no x4 gain in U itself), both with the same N x N taps.
// One 256-thread workgroup owns one S x S plane at a time: d = known - x goes to LDS, the L down passes and the L up passes run
// between two LDS buffers (S^2 + S^2/4 floats, at most 20 KiB; the taps take 900 bytes more), and x + 4^L r leaves.  The plane's x stays in registers from the
// first read to the last write, so x_out may be x itself.
//
// known restates afd_noise_images' fp32 expression with one IEEE rounding per operation (`noised`): no FMA contraction in this
// file.  The tap sums say fmaf themselves; they follow the general kernels' order (a outer, b inner, ascending), so a result does
// not depend on the launch geometry and is the same from call to call (no atomics).
#include "common.h"

#pragma clang fp contract(off)

#include "diffusion_common.h"

namespace afd {

constexpr int kRefineMaxSide = 64;
constexpr int kRefinePerThread = kRefineMaxSide * kRefineMaxSide / 256;     // elements of a plane per thread, at most

// The tap loops below run over exactly the taps that land inside the plane, their bounds worked out up front, so the loop bodies
// have no branch and the compiler can keep several LDS reads in flight.  K: the taps in LDS.

// dst (s/2 x s/2) = D(src (s x s)), s even
__device__ __forceinline__ void refine_down(const float* __restrict__ src, float* __restrict__ dst, int s, const float* __restrict__ K,
                                            int N) {
  const int lo = (N - 1) / 2, so = s >> 1;
  for (int o = threadIdx.x; o < so * so; o += 256) {
    const int r = o / so, j = o - r * so;
    const int p0 = 2 * r - lo, q0 = 2 * j - lo;                     // tap (a, b) reads src[p0 + a][q0 + b]
    const int a0 = max(0, -p0), a1 = min(N, s - p0), b0 = max(0, -q0), b1 = min(N, s - q0);
    float acc = 0.f;
    for (int a = a0; a < a1; ++a) {
      const float* __restrict__ kr = K + a * N;
      const float* __restrict__ sr = src + (p0 + a) * s + q0;
      for (int b = b0; b < b1; ++b) acc = fmaf(kr[b], sr[b], acc);
    }
    dst[o] = acc;
  }
}

// dst (2c x 2c) = U(src (c x c)): only the taps that land on a sample (an even row and column of the 2x grid) are visited
__device__ __forceinline__ void refine_up(const float* __restrict__ src, float* __restrict__ dst, int c, const float* __restrict__ K,
                                          int N) {
  const int lo = (N - 1) / 2, s = 2 * c;
  for (int o = threadIdx.x; o < s * s; o += 256) {
    const int p = o / s, q = o - p * s;
    const int p0 = p - lo, q0 = q - lo;                             // tap (a, b) reads the 2x grid at [p0 + a][q0 + b]: even ones only
    const int a0 = max((p + lo) & 1, -p0), a1 = min(N, s - p0);     // (-p0 has the parity of p + lo: the first tap stays on a sample)
    const int b0 = max((q + lo) & 1, -q0), b1 = min(N, s - q0);
    float acc = 0.f;
    for (int a = a0; a < a1; a += 2) {
      const float* __restrict__ kr = K + a * N;
      const float* __restrict__ sr = src + ((p0 + a) >> 1) * c;
      for (int b = b0; b < b1; b += 2) acc = fmaf(kr[b], sr[(q0 + b) >> 1], acc);
    }
    dst[o] = acc;
  }
}

// t_prev = t_prev_dev[0] when t_prev_dev is given (graph-replayable), else the host value.  noise may be NULL only when t_prev == 0.
__global__ __launch_bounds__(256) void lowpass_refine_k(const float* x, const float* __restrict__ ref, const float* __restrict__ noise,
                                                        const float* __restrict__ alpha_hat, int t_prev,
                                                        const int64_t* __restrict__ t_prev_dev, Taps t, int N, int L, float gain,
                                                        float* x_out, float* x_out2, long planes, int S) {
  __shared__ float bufA[kRefineMaxSide * kRefineMaxSide];           // sides S, S/4, ...
  __shared__ float bufB[kRefineMaxSide * kRefineMaxSide / 4];       // sides S/2, S/8, ...
  __shared__ float K[AFD_MAX_TAPS * AFD_MAX_TAPS];
  for (int i = threadIdx.x; i < N * N; i += 256) K[i] = t.k[i];      // (the first barrier below orders these writes)
  const int tp = t_prev_dev ? (int)t_prev_dev[0] : t_prev;
  const int SS = S * S;
  Roots k{1.f, 0.f};
  if (tp > 0) k = roots(alpha_hat[tp]);
  for (long plane = blockIdx.x; plane < planes; plane += gridDim.x) {
    const long base = plane * SS;
    float xv[kRefinePerThread];
#pragma unroll
    for (int i = 0; i < kRefinePerThread; ++i) {
      const int e = i * 256 + threadIdx.x;
      if (e < SS) {
        xv[i] = x[base + e];
        const float r = ref[base + e];
        const float known = tp > 0 ? noised(k.sa, k.sb, r, noise[base + e]) : r;
        bufA[e] = known - xv[i];
      }
    }
    __syncthreads();
    float *src = bufA, *dst = bufB;
    int s = S;
    for (int l = 0; l < L; ++l) {                                    // S -> S / 2^L
      refine_down(src, dst, s, K, N);
      __syncthreads();
      float* tmp = src; src = dst; dst = tmp;
      s >>= 1;
    }
    for (int l = 0; l < L; ++l) {                                    // and back: the last pass writes bufA
      refine_up(src, dst, s, K, N);
      __syncthreads();
      float* tmp = src; src = dst; dst = tmp;
      s <<= 1;
    }
#pragma unroll
    for (int i = 0; i < kRefinePerThread; ++i) {
      const int e = i * 256 + threadIdx.x;
      if (e < SS) {
        const float v = xv[i] + gain * src[e];
        x_out[base + e] = v;
        if (x_out2) x_out2[base + e] = v;
      }
    }
    __syncthreads();                                                 // the next plane overwrites bufA
  }
}

static int lowpass_refine_any(const char* name, bool dev, const float* x, const float* ref, const float* noise, const float* alpha_hat,
                              int t_prev, const int64_t* t_prev_dev, const float* taps, int N, int levels, float* x_out,
                              float* x_out2, long planes, int S, afd_stream_t stream) {
  AFD_REQUIRE(x && ref && alpha_hat && taps && x_out && (!dev || t_prev_dev), "%s: x, ref, alpha_hat, %staps and x_out must not be NULL",
              name, dev ? "t_prev_dev, " : "");
  AFD_REQUIRE(planes > 0, "%s: planes must be positive (got %ld)", name, planes);
  AFD_REQUIRE(N >= 1 && N <= AFD_MAX_TAPS && (N & 1), "%s: N must be odd and at most %d (got %d): an even N shifts the image", name,
              AFD_MAX_TAPS, N);
  AFD_REQUIRE(S >= 4 && S <= kRefineMaxSide && (S & (S - 1)) == 0, "%s: S must be a power of two in [4, %d] (got %d)", name,
              kRefineMaxSide, S);
  AFD_REQUIRE(levels >= 1 && levels < 31 && (S >> levels) >= 2, "%s: levels must be at least 1 with S / 2^levels >= 2 (got levels = %d, S = %d)",
              name, levels, S);
  AFD_REQUIRE(dev || t_prev >= 0, "%s: t_prev must not be negative (got %d)", name, t_prev);
  AFD_REQUIRE(noise || (!dev && t_prev == 0), "%s: noise must not be NULL %s(it noises the reference)", name,
              dev ? "" : "when t_prev > 0 ");
  const long fb = planes * S * S * (long)sizeof(float);
  AFD_REQUIRE(!overlaps(x_out, fb, ref, fb) && !overlaps(x_out, fb, noise, fb) &&
                  !(x_out2 && (overlaps(x_out2, fb, ref, fb) || overlaps(x_out2, fb, noise, fb))),
              "%s: ref and noise must not overlap x_out or x_out2", name);
  AFD_REQUIRE((x_out == x || !overlaps(x_out, fb, x, fb)) && !(x_out2 && (overlaps(x_out2, fb, x, fb) || overlaps(x_out2, fb, x_out, fb))),
              "%s: x_out must be x itself or apart from it, and x_out2 must not overlap x or x_out", name);
  const float gain = (float)(1L << (2 * levels));                   // 4^levels: up2's DC gain of 1/4 per level, undone
  Taps t;
  for (int i = 0; i < N * N; ++i) t.k[i] = taps[i];
  const unsigned grid = (unsigned)std::min<long>(planes, 1L << 20);
  hipLaunchKernelGGL(lowpass_refine_k, dim3(grid), dim3(256), 0, as_stream(stream), x, ref, noise, alpha_hat, t_prev, t_prev_dev, t, N,
                     levels, gain, x_out, x_out2, planes, S);
  return check_launch(name);
}

}  // namespace afd

using namespace afd;

extern "C" {

int afd_lowpass_refine(const float* x, const float* ref, const float* noise, const float* alpha_hat, int t_prev, const float* taps, int N,
                       int levels, float* x_out, float* x_out2, long planes, int S, afd_stream_t stream) {
  return lowpass_refine_any("afd_lowpass_refine", false, x, ref, noise, alpha_hat, t_prev, nullptr, taps, N, levels, x_out, x_out2, planes,
                            S, stream);
}

int afd_lowpass_refine_dev(const float* x, const float* ref, const float* noise, const float* alpha_hat, const int64_t* t_prev_dev,
                           const float* taps, int N, int levels, float* x_out, float* x_out2, long planes, int S, afd_stream_t stream) {
  return lowpass_refine_any("afd_lowpass_refine_dev", true, x, ref, noise, alpha_hat, 0, t_prev_dev, taps, N, levels, x_out, x_out2,
                            planes, S, stream);
}

}  // extern "C"

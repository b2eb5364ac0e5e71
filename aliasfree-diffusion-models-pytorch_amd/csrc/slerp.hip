// slerp.hip -- spherical interpolation of latent rows (Diffusion.interpolate).
//
// One workgroup per (pair, weight).  It holds its pair's two rows in registers (at most 12 quads of each per thread), takes the
// three sums d = sum a_i b_i, na = sum a_i^2, nb = sum b_i^2 in fp64 out of those registers, and writes its own output row from
// them: a and b are read once per workgroup and nothing is read twice.  The W workgroups of a pair repeat the sums; they run in
// the same fixed order, so they get the same bits, and the repeated reads of a row of at most 48 KB come out of L2.  One
// workgroup per pair would save them and leave most of the chip idle at the sizes this is used at (a few pairs, a few weights).
//
// The order of the sums depends on the row length alone: element i belongs to thread (i / 4) % 256, a thread adds its elements
// in ascending i, a shuffle tree adds the lanes of a wave, the four waves are added in wave order.  The 16-byte and the scalar
// path load differently and add alike, so alignment does not change a bit either.  No atomics.
#include "common.h"

#pragma clang fp contract(off)

#include "diffusion_common.h"

namespace afd {

constexpr int kSlerpThreads = 256;
constexpr long kSlerpMaxRow = 3 * 64 * 64;                                   // C * H * W of the largest latent
constexpr int kSlerpQuads = (int)(kSlerpMaxRow / 4 / kSlerpThreads);        // quads of a row per thread
static_assert((long)kSlerpQuads * 4 * kSlerpThreads == kSlerpMaxRow, "a full row is whole quads per thread");

// In fp64: c = clamp(d / sqrt(na nb), -1, 1), omega = acos(c), so = sin(omega);
//   na == 0, nb == 0 or so < 1e-6 (parallel and antiparallel rows):  ca = 1 - w, cb = w           (lerp)
//   otherwise:                                                       ca = sin((1 - w) omega) / so, cb = sin(w omega) / so
// w = 0 gives (so / so, 0 / so) = (1, 0) and w = 1 gives (0, 1) exactly.
__device__ __forceinline__ void slerp_coefficients(double d, double na, double nb, double w, double& ca, double& cb) {
  ca = 1.0 - w;
  cb = w;
  if (na == 0.0 || nb == 0.0) return;
  const double c = fmin(fmax(d / sqrt(na * nb), -1.0), 1.0);
  const double omega = acos(c), so = sin(omega);
  if (so < 1e-6) return;
  ca = sin((1.0 - w) * omega) / so;
  cb = sin(w * omega) / so;
}

// out[pair][wi][i] = (float)(ca * a[pair][i] + cb * b[pair][i]): the two products and the sum in fp64, then one rounding to fp32
template <bool VEC>
__global__ __launch_bounds__(kSlerpThreads) void slerp_rows_k(const float* __restrict__ a, const float* __restrict__ b,
                                                              const float* __restrict__ w, float* __restrict__ out, long W, long row) {
  __shared__ double red[3 * (kSlerpThreads / kWave)];
  __shared__ double coef[2];
  const long pair = blockIdx.x / W, wi = blockIdx.x - pair * W;
  const float *pa = a + pair * row, *pb = b + pair * row;
  float4 va[kSlerpQuads], vb[kSlerpQuads];
  double d = 0.0, na = 0.0, nb = 0.0;
#pragma unroll
  for (int j = 0; j < kSlerpQuads; ++j) {
    const long o = 4 * ((long)threadIdx.x + kSlerpThreads * j), left = row - o;
    va[j] = vb[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (left > 0) {
      va[j] = load_quad<VEC>(pa, o, left);               // (lanes past the row's end are zero: they add +0)
      vb[j] = load_quad<VEC>(pb, o, left);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double x = lane(va[j], q), y = lane(vb[j], q);
        d += x * y;
        na += x * x;
        nb += y * y;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    d += __shfl_down(d, o, kWave);
    na += __shfl_down(na, o, kWave);
    nb += __shfl_down(nb, o, kWave);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[3 * wave] = d;
    red[3 * wave + 1] = na;
    red[3 * wave + 2] = nb;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < kSlerpThreads / kWave; ++i) {
      d += red[3 * i];
      na += red[3 * i + 1];
      nb += red[3 * i + 2];
    }
    slerp_coefficients(d, na, nb, (double)w[wi], coef[0], coef[1]);
  }
  __syncthreads();
  const double ca = coef[0], cb = coef[1];
  float* po = out + (pair * W + wi) * row;
#pragma unroll
  for (int j = 0; j < kSlerpQuads; ++j) {
    const long o = 4 * ((long)threadIdx.x + kSlerpThreads * j), left = row - o;
    if (left > 0)
      store_quad<VEC>(po, o, left, quad_map([=](float x, float y) {
                        const double l = ca * (double)x, r = cb * (double)y;
                        return (float)(l + r);
                      }, va[j], vb[j]));
  }
}

}  // namespace afd
using namespace afd;

extern "C" {

int afd_slerp_rows(const float* a, const float* b, const float* w, float* out, long pairs, long W, long row, afd_stream_t st) {
  AFD_REQUIRE(a && b && w && out, "afd_slerp_rows: a, b, w and out must not be NULL");
  AFD_REQUIRE(pairs > 0 && W > 0 && row > 0, "afd_slerp_rows: pairs, W and row must be positive (got %ld, %ld, %ld)", pairs, W, row);
  AFD_REQUIRE(row <= kSlerpMaxRow, "afd_slerp_rows: a row holds at most %ld values (got %ld)", kSlerpMaxRow, row);
  AFD_REQUIRE(pairs <= 0x7fffffffL / W, "afd_slerp_rows: at most 2^31 - 1 output rows per call (got %ld x %ld)", pairs, W);
  AFD_REQUIRE((((uintptr_t)a | (uintptr_t)b | (uintptr_t)w | (uintptr_t)out) & 3) == 0, "afd_slerp_rows: a, b, w and out must be 4-byte aligned");
  const long fb = (long)sizeof(float), in = pairs * row * fb, ob = pairs * W * row * fb;
  AFD_REQUIRE(!overlaps(out, ob, a, in) && !overlaps(out, ob, b, in) && !overlaps(out, ob, w, W * fb),
              "afd_slerp_rows: out must not overlap a, b or w");
  launch_vec(vec_ok(row, {a, b, out}), slerp_rows_k<true>, slerp_rows_k<false>, pairs * W, as_stream(st), a, b, w, out, W, row);
  return check_launch("afd_slerp_rows");
}

}  // extern "C"

// analytic.hip -- Analytic-DPM (Bao et al. 2022): the per-row squared norm of a batch of eps predictions, the statistic whose
// per-timestep mean G_t = E|eps_theta(x_t, t)|^2 / d gives the optimal reverse variance in closed form (analytic.py builds the
// table and the sigmas from it; the step that uses them is DdimVar in sampler.hip).  DESIGN.md section 6zd has the derivation.
//
// The guided form builds eps by the step kernels' own fp32 expression (diffusion_common.h), so the pragma below holds here as it
// does in sampler.hip; the squares and every sum are fp64 in a fixed order.
#include "common.h"

#pragma clang fp contract(off)

#include "diffusion_common.h"

namespace afd {

// One workgroup per row b, thread i takes the quads i, i + 256, ... of the row and their elements in index order; the VEC form
// (chw % 4 == 0, a 16-byte aligned pointer) reads the same quads with one 128-bit access, so both forms add the same values in
// the same order.  kCfg: eps holds 2B rows, the conditional half first, and e is guided_eps of the two.
//   rows[b] = sum_i (double)e_i * (double)e_i
template <bool kCfg, bool VEC>
__global__ __launch_bounds__(256) void eps_sqnorm_rows_k(const float* __restrict__ eps, float s, double* __restrict__ rows, long B,
                                                         long chw) {
  __shared__ double red[8];
  const long o = (long)blockIdx.x * chw, ou = o + B * chw;
  const Guidance g = guidance(s);
  double sum = 0.0, unused = 0.0;
  for (long q = threadIdx.x; 4 * q < chw; q += 256) {
    const long left = chw - 4 * q;
    const float4 c = load_quad<VEC>(eps, o + 4 * q, left);
    const float4 u = kCfg ? load_quad<VEC>(eps, ou + 4 * q, left) : c;
    const float4 e = quad_map([&](float ci, float ui) { return guided_eps<kCfg>(g, ci, ui); }, c, u);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i < left) {
        const double ei = (double)lane(e, i);
        sum += ei * ei;
      }
    }
  }
  block_sum2_f64(sum, unused, red);
  if (threadIdx.x == 0) rows[blockIdx.x] = sum;
}

template <bool kCfg>
static int launch_eps_sqnorm_rows(const char* name, const float* eps, float s, double* rows, long B, long chw, hipStream_t st) {
  AFD_REQUIRE(eps && rows, "%s: %s and rows must not be NULL", name, kCfg ? "eps2" : "eps");
  AFD_REQUIRE(B > 0 && chw > 0, "%s: B and chw must be positive (got %ld, %ld)", name, B, chw);
  AFD_REQUIRE(B <= 0x7fffffffL, "%s: at most 2^31 - 1 rows per call (got %ld)", name, B);
  AFD_REQUIRE(!overlaps(rows, B * (long)sizeof(double), eps, (kCfg ? 2 : 1) * B * chw * (long)sizeof(float)),
              "%s: rows must not overlap the input", name);
  // the second half of eps2 starts B * chw floats on: 16-byte aligned whenever eps2 is and chw % 4 == 0
  launch_vec(vec_ok(chw, {eps}), eps_sqnorm_rows_k<kCfg, true>, eps_sqnorm_rows_k<kCfg, false>, B, st, eps, s, rows, B, chw);
  return check_launch(name);
}

}  // namespace afd
using namespace afd;

extern "C" {

int afd_eps_sqnorm_rows(const float* eps, double* rows, long B, long chw, afd_stream_t st) {
  return launch_eps_sqnorm_rows<false>("afd_eps_sqnorm_rows", eps, 0.0f, rows, B, chw, as_stream(st));
}
int afd_eps_sqnorm_rows_cfg(const float* eps2, float cfg_scale, double* rows, long B, long chw, afd_stream_t st) {
  return launch_eps_sqnorm_rows<true>("afd_eps_sqnorm_rows_cfg", eps2, cfg_scale, rows, B, chw, as_stream(st));
}

}  // extern "C"

// likelihood.hip -- the two launches of Diffusion.ode_likelihood, the model's log-density from the probability-flow ODE with a
// Hutchinson trace (Song et al. 2021, section 4.3): the per-row fp64 reduction that adds one evaluation's
// trace estimate (and, at the end, the prior's -|x_U|^2 / 2) into an accumulator, and the corrector of Heun's rule.
//
// afd_ode_trace_rows: one 256-thread workgroup per row.  The order of a row's sums depends on the row length alone: element i
// belongs to thread (i / 4) % 256, a thread adds its elements in ascending i, a shuffle tree adds the lanes of a wave, the four
// waves are added in wave order, and thread 0 alone reads, updates and writes acc[row].  The 16-byte and the scalar path load
// differently and add alike.  Products are formed in fp64, where the product of two fp32 values is exact.  No atomics, no
// workspace: the same bits from call to call.  A few rows leave most of the chip idle; the launch sits beside a forward and a
// backward of the network (as afd_dps_residual's does).
//
// afd_ode_heun_step: elementwise fp32, one IEEE rounding per operation (no contraction in this file).
#include "common.h"

#pragma clang fp contract(off)

#include "diffusion_common.h"

namespace afd {

constexpr int kTraceThreads = 256;

// acc[row] = acc[row] + ((cvv * sum_j v^2) + (cvw * sum_j v w)); without w: acc[row] + (cvv * sum_j v^2)
template <bool VEC, bool HAS_W>
__global__ __launch_bounds__(kTraceThreads) void ode_trace_rows_k(const float* __restrict__ v, const float* __restrict__ w, double cvv,
                                                                  double cvw, double* __restrict__ acc, long per) {
  __shared__ double red[2 * (kTraceThreads / kWave)];
  const long row = blockIdx.x;
  const float* pv = v + row * per;
  const float* pw = HAS_W ? w + row * per : nullptr;
  double svv = 0.0, svw = 0.0;
  for (long o = 4 * (long)threadIdx.x; o < per; o += 4 * kTraceThreads) {
    const long left = per - o;
    const float4 a = load_quad<VEC>(pv, o, left);                   // (lanes past the row's end are zero: they add +0)
    const float4 b = HAS_W ? load_quad<VEC>(pw, o, left) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double x = lane(a, q);
      svv += x * x;
      if (HAS_W) svw += x * (double)lane(b, q);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    svv += __shfl_down(svv, o, kWave);
    if (HAS_W) svw += __shfl_down(svw, o, kWave);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[2 * wave] = svv;
    red[2 * wave + 1] = svw;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < kTraceThreads / kWave; ++i) {
      svv += red[2 * i];
      svw += red[2 * i + 1];
    }
    const double l = cvv * svv;
    acc[row] = acc[row] + (HAS_W ? l + cvw * svw : l);
  }
}

// x_out = sqrt(a_u) * ((x / sqrt(a_s)) + ((h / 2) * (eps_s + eps_u))), h in fp64 from the fp32 table and rounded once
template <bool VEC>
__global__ __launch_bounds__(256) void ode_heun_step_k(const float* x, const float* __restrict__ eps_s, const float* __restrict__ eps_u,
                                                       const float* __restrict__ alpha_hat, int s, int u, float* x_out, long n) {
  const float a_s = alpha_hat[s], a_u = alpha_hat[u];
  const float sq_as = sqrtf(a_s), sq_au = sqrtf(a_u);
  const double das = (double)a_s, dau = (double)a_u;
  const float h = (float)(sqrt((1.0 - dau) / dau) - sqrt((1.0 - das) / das));
  const float hh = 0.5f * h;                                        // exact
  auto rule = [=](float xi, float es, float eu) {
    const float y = xi / sq_as;
    const float m = es + eu;
    const float d = hh * m;
    return sq_au * (y + d);
  };
  AFD_GRID_STRIDE(i, n) {
    if (VEC) {
      const float4 xv = reinterpret_cast<const float4*>(x)[i];
      const float4 es = reinterpret_cast<const float4*>(eps_s)[i], eu = reinterpret_cast<const float4*>(eps_u)[i];
      reinterpret_cast<float4*>(x_out)[i] = quad_map(rule, xv, es, eu);
    } else {
      x_out[i] = rule(x[i], eps_s[i], eps_u[i]);
    }
  }
}

}  // namespace afd
using namespace afd;

extern "C" {

int afd_ode_trace_rows(const float* v, const float* w, double cvv, double cvw, double* acc, long rows, long per, afd_stream_t st) {
  const char* name = "afd_ode_trace_rows";
  AFD_REQUIRE(v && acc, "%s: v and acc must not be NULL", name);
  AFD_REQUIRE(std::isfinite(cvv) && std::isfinite(cvw), "%s: cvv and cvw must be finite (got %g, %g)", name, cvv, cvw);
  AFD_REQUIRE(w || cvw == 0.0, "%s: w must not be NULL unless cvw == 0 (got cvw = %g)", name, cvw);
  AFD_REQUIRE(rows > 0 && per > 0, "%s: rows and per must be positive (got %ld, %ld)", name, rows, per);
  AFD_REQUIRE(rows <= 0x7fffffffL && per <= (1L << 40) / rows, "%s: at most 2^31 - 1 rows and 2^40 values per call (got %ld x %ld)", name,
              rows, per);
  AFD_REQUIRE((((uintptr_t)v | (uintptr_t)w) & 3) == 0 && ((uintptr_t)acc & 7) == 0, "%s: v and w must be 4-byte, acc 8-byte aligned", name);
  const long fb = rows * per * (long)sizeof(float), ab = rows * (long)sizeof(double);
  AFD_REQUIRE(!overlaps(acc, ab, v, fb) && !overlaps(acc, ab, w, fb), "%s: acc must not overlap v or w", name);
  const bool vec = vec_ok(per, {v, w});
  if (w)
    launch_vec(vec, ode_trace_rows_k<true, true>, ode_trace_rows_k<false, true>, rows, as_stream(st), v, w, cvv, cvw, acc, per);
  else
    launch_vec(vec, ode_trace_rows_k<true, false>, ode_trace_rows_k<false, false>, rows, as_stream(st), v, w, cvv, cvw, acc, per);
  return check_launch(name);
}

int afd_ode_heun_step(const float* x, const float* eps_s, const float* eps_u, const float* alpha_hat, int s, int u, float* x_out, long n,
                      afd_stream_t st) {
  const char* name = "afd_ode_heun_step";
  AFD_REQUIRE(x && eps_s && eps_u && alpha_hat && x_out, "%s: x, eps_s, eps_u, alpha_hat and x_out must not be NULL", name);
  AFD_REQUIRE(n > 0, "%s: n must be positive (got %ld)", name, n);
  AFD_REQUIRE(s >= 1 && s < u, "%s: need 1 <= s < u (got s = %d, u = %d)", name, s, u);
  const long fb = n * (long)sizeof(float);
  AFD_REQUIRE(!overlaps(x_out, fb, eps_s, fb) && !overlaps(x_out, fb, eps_u, fb), "%s: x_out must not overlap eps_s or eps_u", name);
  AFD_REQUIRE(x_out == x || !overlaps(x_out, fb, x, fb), "%s: x_out must be x itself or apart from it", name);
  const bool vec = vec_ok(n, {x, eps_s, eps_u, x_out});
  const long work = vec ? n / 4 : n;
  const long grid = std::min<long>(2048, std::max<long>(1, (work + 255) / 256));
  launch_vec(vec, ode_heun_step_k<true>, ode_heun_step_k<false>, grid, as_stream(st), x, eps_s, eps_u, alpha_hat, s, u, x_out, work);
  return check_launch(name);
}

}  // extern "C"

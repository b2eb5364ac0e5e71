// tsampler.hip -- loss-aware timestep sampling (Nichol & Dhariwal 2021, "loss-second-moment resampling"), on the device:
// the per-row losses of a batch, the sampler's tick (fold the batch into the per-timestep history, rebuild the distribution and
// the importance-weight tables the loss kernels read) and the draw.  DESIGN.md section 6m has the semantics.
//
// The row losses form pred - target by the loss kernels' own fp32 expressions (objective_common.h), so the pragma below holds
// here as it does in objective.hip; everything after that difference, and the whole tick, is fp64 in a fixed order.
#include "common.h"

#pragma clang fp contract(off)

#include "objective_common.h"

namespace afd {

// ---- per-row losses -------------------------------------------------------------------------------------------------------------
// One workgroup per row b, thread i takes the quads i, i + 256, ... of the row and their elements in index order; the VEC form
// (chw % 4 == 0, 16-byte aligned pointers) reads the same quads with one 128-bit access per stream, so both forms add the same
// values in the same order.  LVAR: out holds rows of 2 chw floats (the prediction, then the variance coefficient).
//   rows[b] = (1 / chw) w[t_b] sum_i (double)d_i^2,  d_i = objective_diff in fp32           (L_simple's share of row b, times B)
//           + (vlb_scale / (chw ln 2)) sum_i lvar_term_i                                      (LVAR: the bound's share)
template <bool LVAR, bool VEC>
__global__ __launch_bounds__(256) void loss_rows_k(const float* __restrict__ out, const float* __restrict__ x0,
                                                   const float* __restrict__ eps, const int64_t* __restrict__ t,
                                                   const float* __restrict__ alpha, const float* __restrict__ alpha_hat,
                                                   const float* __restrict__ beta, const double* __restrict__ lv_coef,
                                                   const float* __restrict__ w, int kind, double vlb_scale,
                                                   double* __restrict__ rows, long chw) {
  __shared__ double red[8];
  const long b = blockIdx.x;
  const long tb = t[b];
  const Roots k = roots(alpha_hat[tb]);
  LvarRow row;
  if (LVAR) row = lvar_row(lv_coef, alpha, alpha_hat, beta, tb, kind);
  const long o = b * chw, o2 = LVAR ? 2 * b * chw : o;
  double s = 0.0, sv = 0.0;
  for (long q = threadIdx.x; 4 * q < chw; q += 256) {
    const long left = chw - 4 * q;
    const float4 p = load_quad<VEC>(out, o2 + 4 * q, left);
    const float4 x = LVAR || kind != AFD_PRED_EPS ? load_quad<VEC>(x0, o + 4 * q, left) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 e = LVAR || kind != AFD_PRED_X0 ? load_quad<VEC>(eps, o + 4 * q, left) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 v = LVAR ? load_quad<VEC>(out, o2 + chw + 4 * q, left) : p;
    const float4 d = objective_diff4(kind, p, x, e, k);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i < left) {
        const double di = (double)lane(d, i);
        s += di * di;
        if (LVAR) {
          double sq, dlv;
          sv += lvar_term<false>(row, kind, lane(p, i), lane(v, i), lane(x, i), lane(e, i),
                                 noised(k.sa, k.sb, lane(x, i), lane(e, i)), sq, dlv);
        }
      }
    }
  }
  block_sum2_f64(s, sv, red);
  if (threadIdx.x == 0) {
    const double wb = w ? (double)w[tb] : 1.0;
    double r = (wb * s) / (double)chw;
    if (LVAR) r += (vlb_scale / ((double)chw * 0.6931471805599453)) * sv;
    rows[b] = r;
  }
}

// ---- the tick: update + refresh, one workgroup -------------------------------------------------------------------------------------
// The sum of v over the workgroup's 256 threads, in a fixed order, in every thread.  red: 4 doubles of LDS.
__device__ __forceinline__ double block_sum_f64_all(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, kWave);
  __syncthreads();                                    // (red may still be read from the call before)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// hist (T, H) fp64 and count (T) are the state; prob (T), cdf (T - lo), wtab (T), vwtab (T, optional) and warm[0] are rebuilt.
// Thread i owns the timesteps i, i + 256, ...: it alone touches their histories, so scanning the batch in order reproduces the
// sequential update without atomics (a row whose t lies outside [0, T) or whose loss is not finite is skipped).
__global__ __launch_bounds__(256) void tsampler_tick_k(const int64_t* __restrict__ t, const double* __restrict__ rows, long B,
                                                       double* __restrict__ hist, int* __restrict__ count, long T, long H, long lo,
                                                       double uniform_prob, const float* __restrict__ w_base,
                                                       double* __restrict__ prob, double* __restrict__ cdf,
                                                       float* __restrict__ wtab, float* __restrict__ vwtab, int* __restrict__ warm) {
  __shared__ double red[4];
  __shared__ double chunk_off[257];
  const long tid = threadIdx.x;
  // update: the batch's timesteps pass through LDS 256 at a time, every thread walks them in batch order
  __shared__ long t_sh[256];
  for (long base = 0; base < B; base += 256) {
    __syncthreads();
    if (base + tid < B) t_sh[tid] = t[base + tid];
    __syncthreads();
    const int m = (int)(B - base < 256 ? B - base : 256);
    for (int i = 0; i < m; ++i) {
      const long tb = t_sh[i];
      if (tb < 0 || tb >= T || (tb & 255) != tid) continue;
      const double l = rows[base + i];
      if (!isfinite(l)) continue;
      double* h = hist + tb * H;
      const int c = count[tb];
      if (c >= H) {
        for (long j = 0; j + 1 < H; ++j) h[j] = h[j + 1];
        h[H - 1] = l;
      } else {
        h[c] = l;
        count[tb] = c + 1;
      }
    }
  }
  // refresh: q_t = sqrt(mean_j hist[t][j]^2) of the timesteps this thread owns (kept in prob until p_t replaces it)
  const long n = T - lo;
  double sq = 0.0, not_full = 0.0;
  for (long ts = tid; ts < T; ts += 256) {
    if (ts < lo) continue;
    const double* h = hist + ts * H;
    double m = 0.0;
    for (long j = 0; j < H; ++j) m += h[j] * h[j];
    const bool full = count[ts] >= H;
    const double q = full ? sqrt(m / (double)H) : 0.0;
    prob[ts] = q;
    sq += q;
    if (!full) not_full += 1.0;
  }
  const double sum_q = block_sum_f64_all(sq, red);
  const bool is_warm = block_sum_f64_all(not_full, red) == 0.0;
  const bool weighted = is_warm && sum_q > 0.0 && isfinite(sum_q);
  const double uni = 1.0 / (double)n;
  for (long ts = tid; ts < T; ts += 256) {
    double p = 0.0, iw = 1.0;
    if (ts >= lo) {
      if (weighted) {
        const double l = (prob[ts] / sum_q) * (1.0 - uniform_prob), r = uniform_prob / (double)n;
        p = l + r;
        iw = 1.0 / ((double)n * p);
      } else {
        p = uni;
      }
    }
    prob[ts] = p;
    wtab[ts] = (float)((w_base ? (double)w_base[ts] : 1.0) * iw);
    if (vwtab) vwtab[ts] = (float)iw;
  }
  if (tid == 0) warm[0] = is_warm ? 1 : 0;
  __syncthreads();                                    // prob is complete, for every thread of the workgroup
  // cdf: thread i sums the contiguous chunk i of p over [lo, T), thread 0 turns the 256 chunk sums into offsets one after the
  // other, and every prefix is offset + the running sum of its chunk: a fixed order, and non-decreasing across chunk borders
  // (the last prefix of a chunk is the next chunk's offset, bit for bit)
  const long per = (n + 255) / 256;
  const long k0 = tid * per < n ? tid * per : n, k1 = k0 + per < n ? k0 + per : n;
  double run = 0.0;
  for (long k = k0; k < k1; ++k) run += prob[lo + k];
  chunk_off[tid + 1] = run;
  __syncthreads();
  if (tid == 0) {
    chunk_off[0] = 0.0;
    for (int i = 1; i <= 256; ++i) chunk_off[i] = chunk_off[i - 1] + chunk_off[i];
  }
  __syncthreads();
  const double total = chunk_off[256], off = chunk_off[tid];
  run = 0.0;
  for (long k = k0; k < k1; ++k) {
    run += prob[lo + k];
    cdf[k] = k == n - 1 ? 1.0 : (off + run) / total;
  }
}

// t_out[b] = lo + the first k in [0, n) with u[b] < cdf[k] (numpy's searchsorted(cdf, u, side="right")), clamped to n - 1
__global__ __launch_bounds__(256) void tsampler_draw_k(const double* __restrict__ cdf, const double* __restrict__ u, long lo, long n,
                                                       int64_t* __restrict__ t_out, long B) {
  AFD_GRID_STRIDE(b, B) {
    const double ub = u[b];
    long a = 0, e = n;                                // the answer lies in [a, e]
    while (a < e) {
      const long m = a + (e - a) / 2;
      if (ub < cdf[m]) e = m;
      else a = m + 1;
    }
    t_out[b] = lo + (a < n - 1 ? a : n - 1);
  }
}

}  // namespace afd
using namespace afd;

template <bool LVAR>
static int launch_loss_rows(const char* name, const float* out, const float* x0, const float* eps, const int64_t* t, const float* alpha,
                            const float* alpha_hat, const float* beta, const double* lv_coef, const float* w, int kind,
                            double vlb_scale, double* rows, long B, long chw, hipStream_t st) {
  AFD_REQUIRE_KIND(name, kind);
  AFD_REQUIRE_B_CHW(name, B, chw);
  AFD_REQUIRE(B <= 0x7fffffffL, "%s: at most 2^31 - 1 rows per call (got %ld)", name, B);
  const long fb = B * chw * (long)sizeof(float), db = B * (long)sizeof(double);
  AFD_REQUIRE(!overlaps(rows, db, out, (LVAR ? 2 : 1) * fb) && !overlaps(rows, db, x0, fb) && !overlaps(rows, db, eps, fb) &&
                  !overlaps(rows, db, t, B * (long)sizeof(int64_t)),
              "%s: rows must not overlap an input", name);
  launch_vec(vec_ok(chw, {out, x0, eps}), loss_rows_k<LVAR, true>, loss_rows_k<LVAR, false>, B, st, out, x0, eps, t, alpha, alpha_hat,
             beta, lv_coef, w, kind, vlb_scale, rows, chw);
  return check_launch(name);
}

extern "C" {

int afd_loss_rows(const float* pred, const float* x0, const float* eps, const int64_t* t, const float* alpha_hat, const float* w,
                  int kind, double* rows, long B, long chw, afd_stream_t st) {
  AFD_REQUIRE(pred && x0 && eps && t && alpha_hat && rows, "afd_loss_rows: pred, x0, eps, t, alpha_hat and rows must not be NULL");
  return launch_loss_rows<false>("afd_loss_rows", pred, x0, eps, t, nullptr, alpha_hat, nullptr, nullptr, w, kind, 0.0, rows, B, chw,
                                 as_stream(st));
}
int afd_lvar_loss_rows(const float* out2, const float* x0, const float* eps, const int64_t* t, const float* alpha,
                       const float* alpha_hat, const float* beta, const double* lv_coef, const float* w, int kind, double vlb_scale,
                       double* rows, long B, long chw, afd_stream_t st) {
  AFD_REQUIRE(out2 && x0 && eps && t && alpha && alpha_hat && beta && lv_coef && rows,
              "afd_lvar_loss_rows: out2, x0, eps, t, alpha, alpha_hat, beta, lv_coef and rows must not be NULL");
  AFD_REQUIRE_VLB_SCALE("afd_lvar_loss_rows", vlb_scale);
  return launch_loss_rows<true>("afd_lvar_loss_rows", out2, x0, eps, t, alpha, alpha_hat, beta, lv_coef, w, kind, vlb_scale, rows, B,
                                chw, as_stream(st));
}

int afd_tsampler_tick(const int64_t* t, const double* rows, long B, double* hist, int* count, long T, long H, long lo,
                      double uniform_prob, const float* w_base, double* prob, double* cdf, float* wtab, float* vwtab, int* warm,
                      afd_stream_t st) {
  AFD_REQUIRE(t && rows && hist && count && prob && cdf && wtab && warm,
              "afd_tsampler_tick: t, rows, hist, count, prob, cdf, wtab and warm must not be NULL");
  AFD_REQUIRE(B > 0 && T > 0 && H >= 1, "afd_tsampler_tick: B and T must be positive and H >= 1 (got %ld, %ld, %ld)", B, T, H);
  AFD_REQUIRE(lo >= 0 && lo < T, "afd_tsampler_tick: lo must lie in [0, T) (got %ld, T = %ld)", lo, T);
  AFD_REQUIRE(uniform_prob >= 0.0 && uniform_prob < 1.0, "afd_tsampler_tick: uniform_prob must lie in [0, 1) (got %g)", uniform_prob);
  hipLaunchKernelGGL(tsampler_tick_k, dim3(1), dim3(256), 0, as_stream(st), t, rows, B, hist, count, T, H, lo, uniform_prob, w_base,
                     prob, cdf, wtab, vwtab, warm);
  return check_launch("afd_tsampler_tick");
}

int afd_tsampler_draw(const double* cdf, const double* u, long lo, long T, int64_t* t_out, long B, afd_stream_t st) {
  AFD_REQUIRE(cdf && u && t_out, "afd_tsampler_draw: cdf, u and t_out must not be NULL");
  AFD_REQUIRE(B > 0 && T > 0, "afd_tsampler_draw: B and T must be positive (got %ld, %ld)", B, T);
  AFD_REQUIRE(lo >= 0 && lo < T, "afd_tsampler_draw: lo must lie in [0, T) (got %ld, T = %ld)", lo, T);
  hipLaunchKernelGGL(tsampler_draw_k, dim3(gs_grid(B)), dim3(256), 0, as_stream(st), cdf, u, lo, T - lo, t_out, B);
  return check_launch("afd_tsampler_draw");
}

}  // extern "C"

// fidelity.hip -- the two fp64 contractions behind FID and KID, on the fp64 matrix pipe
// (mfma_f64_16x16x4_f64), each with its reduction fused behind it so that the contraction's output never reaches memory:
//   afd_feature_moments_f32   sum_r x_r and sum_r x_r x_r^T of (n, D) fp32 features: the mean and covariance of a feature set
//   afd_poly_mmd_sums_f32     per subset the three sums of a polynomial kernel over gathered rows: the unbiased MMD^2 of KID
// Both work on the 64 x 64 output tiles of f64_tile.h.  The operands are widened from fp32 to fp64 while they are staged into LDS
// as s[k][row], 32 k at a time; rows and k beyond the arrays are zeros in the OPERANDS (a masked load), and the epilogues leave
// padded results out with a select, never a multiplication, so a NaN stays where it belongs.  Partials go to the workspace and a
// second kernel folds them in a fixed order: no atomics, no memset, nothing depends on the order in which workgroups run, so the
// same arguments give the same bits.
#include "f64_tile.h"

namespace afd {

constexpr int kMomPitch = 80;                      // moments: s[k][column]; the four k of a fragment lie 32 banks apart
constexpr int kMmdPitch = 65;                      // MMD: written k-fastest (32 consecutive k of one row: 32 distinct bank pairs)
constexpr long kMomTarget = 2048;                  // workgroups the moments aim for, whatever the device
constexpr long kMomMaxSlabs = 64;
constexpr long kMmdMaxM = 1L << 16;

// pair p of the upper triangle of a T x T grid, rows first: (0, 0), (0, 1), ..., (0, T - 1), (1, 1), ...
__device__ __forceinline__ void fd_pair(long p, int T, int& ti, int& tj) {
  int i = 0;
  long left = p;
  while (left >= T - i) {
    left -= T - i;
    ++i;
  }
  ti = i;
  tj = i + (int)left;
}

// ---- moments ---------------------------------------------------------------------------------------------------------------------
// Workgroup (pair, slab g) walks rows [g per, min(n, (g + 1) per)) of X and leaves the 64 x 64 tile (ti, tj), ti <= tj, of
// sum_r x_r x_r^T in ws[(pair G + g)][64][64]; a diagonal workgroup also leaves the column sums of its 64 columns, summed row by
// row in index order, in the sums part of the workspace, [(ti G + g)][64].
__global__ __launch_bounds__(kTileThreads) void moments_k(const float* __restrict__ X, long n, int D, int T, long per, long G,
                                                        double* __restrict__ ws, double* __restrict__ ws_sum) {
  __shared__ double sa[kTileK * kMomPitch], sb[kTileK * kMomPitch];
  const int tid = threadIdx.x;
  const TileLane q = tile_lane(tid);
  const long pair = blockIdx.x / G, g = blockIdx.x - pair * G;
  int ti, tj;
  fd_pair(pair, T, ti, tj);
  const bool diag = ti == tj;
  const int I = ti * kTile, J = tj * kTile;
  const long r_begin = g * per, r_end = r_begin + per < n ? r_begin + per : n;
  v4d acc[2][2];
  tile_zero(acc);
  double colsum = 0.0;
  const double* sbp = diag ? sa : sb;

  // the thread's elements of a round are (k, c) = (e >> 6, e & 63), e = tid + 256 j; the next round's are loaded into registers
  // while the matrix pipe works on this one
  float na_[kTilePer], nb_[kTilePer];
  auto fetch = [&](long r0) {
#pragma unroll
    for (int j = 0; j < kTilePer; ++j) {
      const int e = tid + kTileThreads * j, c = e & 63;
      const long r = r0 + (e >> 6);
      const bool rok = r < r_end;
      na_[j] = (rok && I + c < D) ? X[r * D + I + c] : 0.0f;
      if (!diag) nb_[j] = (rok && J + c < D) ? X[r * D + J + c] : 0.0f;
    }
  };
  fetch(r_begin);
  for (long r0 = r_begin; r0 < r_end; r0 += kTileK) {
#pragma unroll
    for (int j = 0; j < kTilePer; ++j) {
      const int e = tid + kTileThreads * j, k = e >> 6, c = e & 63;
      sa[k * kMomPitch + c] = (double)na_[j];
      if (!diag) sb[k * kMomPitch + c] = (double)nb_[j];
    }
    __syncthreads();
    if (r0 + kTileK < r_end) fetch(r0 + kTileK);
    tile_round<kMomPitch>(sa, sbp, q, acc);
    if (diag && tid < kTile) {
#pragma unroll 8
      for (int k = 0; k < kTileK; ++k) colsum += sa[k * kMomPitch + tid];
    }
    __syncthreads();
  }

  double* out = ws + (pair * G + g) * (long)(kTile * kTile);
  tile_for_each(q, acc, [&](int row, int col, double v) { out[row * kTile + col] = v; });
  if (diag && tid < kTile) ws_sum[((long)ti * G + g) * kTile + tid] = colsum;
}

// Workgroup `pair` folds the G slabs of its tile in slab order, adds what outer held (accumulate) and writes the element and its
// mirror image from one value, so outer is symmetric bit for bit.  A diagonal tile is taken from its upper half alone.  Only
// elements on or above the diagonal are ever read, and only by the thread that writes them.
__global__ __launch_bounds__(kTileThreads) void moments_finish_k(const double* __restrict__ ws, const double* __restrict__ ws_sum, int D, int T, long G,
                                                               int accumulate, double* __restrict__ sum, double* __restrict__ outer) {
  const int tid = threadIdx.x;
  const long pair = blockIdx.x;
  int ti, tj;
  fd_pair(pair, T, ti, tj);
  const int I = ti * kTile, J = tj * kTile;
  const double* p = ws + pair * G * (long)(kTile * kTile);
  for (int e = tid; e < kTile * kTile; e += kTileThreads) {
    const int gi = I + (e >> 6), gj = J + (e & 63);
    if (gi >= D || gj >= D || gi > gj) continue;
    double v = p[e];
    for (long g = 1; g < G; ++g) v += p[g * (kTile * kTile) + e];
    if (accumulate) v = outer[(long)gi * D + gj] + v;
    outer[(long)gi * D + gj] = v;
    outer[(long)gj * D + gi] = v;
  }
  if (ti == tj && tid < kTile && I + tid < D) {
    const double* q = ws_sum + (long)ti * G * kTile + tid;
    double v = q[0];
    for (long g = 1; g < G; ++g) v += q[g * kTile];
    sum[I + tid] = accumulate ? sum[I + tid] + v : v;
  }
}

static bool mom_sizes_ok(long n, long D) { return n > 0 && D > 0 && n < (1L << 31) && D <= (1L << 15) && D <= (1L << 40) / n; }
static long mom_tiles(long D) { return (D + kTile - 1) / kTile; }
static long mom_pairs(long D) { return mom_tiles(D) * (mom_tiles(D) + 1) / 2; }
// the slabs of a call depend on (n, D) alone
static long mom_slabs(long n, long D) {
  long G = kMomTarget / mom_pairs(D);
  const long rounds = (n + kTileK - 1) / kTileK;
  G = G < 1 ? 1 : G;
  G = G > kMomMaxSlabs ? kMomMaxSlabs : G;
  return G > rounds ? rounds : G;
}

// ---- polynomial-kernel MMD sums ----------------------------------------------------------------------------------------------------
// Per subset s the workgroups are: TP = MT (MT + 1) / 2 upper-triangle tiles of the A x A Gram matrix, TP of B x B, MT^2 tiles of
// A x B, MT = ceil(m / 64).  A workgroup gathers its 64 + 64 rows by index, runs the dot products over D, raises the accumulators
// to the power and sums its tile: a symmetric problem's tile above the diagonal counts twice, a diagonal tile leaves i == j out.
// An index outside its array reads nothing: that row is NaN.
__global__ __launch_bounds__(kTileThreads) void mmd_k(const float* __restrict__ A, long na, const float* __restrict__ B, long nb, int D,
                                                    const int64_t* __restrict__ ia, const int64_t* __restrict__ ib, int m, int MT, long per_subset,
                                                    int degree, double gamma, double coef0, double* __restrict__ ws) {
  __shared__ double sa[kTileK * kMmdPitch], sb[kTileK * kMmdPitch];
  __shared__ long rows_a[kTile], rows_b[kTile];
  __shared__ double red[kTileThreads / kWave];
  const int tid = threadIdx.x, lane = tid & 63;
  const TileLane q = tile_lane(tid);
  const long s = blockIdx.x / per_subset, p = blockIdx.x - s * per_subset;
  const long TP = (long)MT * (MT + 1) / 2;
  int which, ti, tj;                                 // 0: A x A, 1: B x B, 2: A x B
  if (p < 2 * TP) {
    which = p < TP ? 0 : 1;
    fd_pair(p - which * TP, MT, ti, tj);
  } else {
    which = 2;
    ti = (int)((p - 2 * TP) / MT);
    tj = (int)((p - 2 * TP) - (long)ti * MT);
  }
  const bool sym = which != 2, diag = sym && ti == tj;
  const float* src_a = which == 1 ? B : A;
  const float* src_b = which == 0 ? A : B;
  const int64_t* ix_a = (which == 1 ? ib : ia) + s * m;
  const int64_t* ix_b = (which == 0 ? ia : ib) + s * m;
  const long lim_a = which == 1 ? nb : na, lim_b = which == 0 ? na : nb;
  const int I = ti * kTile, J = tj * kTile;
  if (tid < kTile) {                               // -1: past the subset (zeros), -2: an index outside the array (NaN)
    long v = -1;
    if (I + tid < m) {
      v = ix_a[I + tid];
      v = (v < 0 || v >= lim_a) ? -2 : v;
    }
    rows_a[tid] = v;
  } else if (tid < 2 * kTile) {
    const int t = tid - kTile;
    long v = -1;
    if (J + t < m) {
      v = ix_b[J + t];
      v = (v < 0 || v >= lim_b) ? -2 : v;
    }
    rows_b[t] = v;
  }
  __syncthreads();
  long my_a[kTilePer], my_b[kTilePer];                   // thread's staged elements: k = tid & 31, rows (tid >> 5) + 8 j
#pragma unroll
  for (int j = 0; j < kTilePer; ++j) {
    my_a[j] = rows_a[(tid >> 5) + 8 * j];
    my_b[j] = rows_b[(tid >> 5) + 8 * j];
  }
  const int k = tid & 31;
  const float qnan = __builtin_nanf("");
  v4d acc[2][2];
  tile_zero(acc);
  const double* sbp = diag ? sa : sb;

  // the next round's elements are loaded into registers while the matrix pipe works on this one
  float na_[kTilePer], nb_[kTilePer];
  auto fetch = [&](int d0) {
    const bool dok = d0 + k < D;
#pragma unroll
    for (int j = 0; j < kTilePer; ++j) {
      na_[j] = my_a[j] == -2 ? qnan : (my_a[j] >= 0 && dok) ? src_a[my_a[j] * D + d0 + k] : 0.0f;
      if (!diag) nb_[j] = my_b[j] == -2 ? qnan : (my_b[j] >= 0 && dok) ? src_b[my_b[j] * D + d0 + k] : 0.0f;
    }
  };
  fetch(0);
  for (int d0 = 0; d0 < D; d0 += kTileK) {
    tile_stage_kfast<kMmdPitch>(sa, tid, na_);
    if (!diag) tile_stage_kfast<kMmdPitch>(sb, tid, nb_);
    __syncthreads();
    if (d0 + kTileK < D) fetch(d0 + kTileK);
    tile_round<kMmdPitch>(sa, sbp, q, acc);
    __syncthreads();
  }

  double part = 0.0;                                 // the lane's elements in a fixed order (tile_for_each's)
  tile_for_each(q, acc, [&](int row, int col, double dot) {
    const int i = I + row, jj = J + col;
    const double v = gamma * dot + coef0;
    double pw = v;
    for (int t = 1; t < degree; ++t) pw *= v;
    if (i < m && jj < m && !(diag && i == jj)) part += pw;
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, kWave);
  if (lane == 0) red[q.w] = part;
  __syncthreads();
  if (tid == 0) {
    const double t = ((red[0] + red[1]) + red[2]) + red[3];
    ws[blockIdx.x] = (sym && !diag) ? 2.0 * t : t;
  }
}

// Wave (s, which) folds its workgroups' partials: the lanes take partials lane, lane + 64, ... in index order, a shuffle tree adds
// the lanes.
__global__ __launch_bounds__(kWave) void mmd_finish_k(const double* __restrict__ ws, int MT, long per_subset, double* __restrict__ sums) {
  const int lane = threadIdx.x;
  const long s = blockIdx.x / 3;
  const int which = (int)(blockIdx.x - 3 * s);
  const long TP = (long)MT * (MT + 1) / 2;
  const long begin = which * TP, count = which == 2 ? (long)MT * MT : TP;
  const double* p = ws + s * per_subset + begin;
  double v = 0.0;
  for (long i = lane; i < count; i += kWave) v += p[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, kWave);
  if (lane == 0) sums[blockIdx.x] = v;
}

static long mmd_tiles(long m) { return (m + kTile - 1) / kTile; }
static long mmd_per_subset(long m) { return mmd_tiles(m) * (mmd_tiles(m) + 1) + mmd_tiles(m) * mmd_tiles(m); }
static bool mmd_sizes_ok(long S, long m, long D) {
  return S > 0 && D > 0 && m >= 2 && m <= kMmdMaxM && D < (1L << 31) && S <= ((1L << 31) - 1) / mmd_per_subset(m);
}

}  // namespace afd
using namespace afd;

extern "C" {

size_t afd_feature_moments_workspace_bytes(long n, long D) {
  if (!mom_sizes_ok(n, D)) return 0;
  const size_t G = (size_t)mom_slabs(n, D);
  return (G * (size_t)mom_pairs(D) * kTile * kTile + G * (size_t)mom_tiles(D) * kTile) * sizeof(double);
}

int afd_feature_moments_f32(const float* X, long n, long D, double* sum, double* outer, int accumulate, void* workspace,
                            size_t workspace_bytes, afd_stream_t st) {
  const char* name = "afd_feature_moments_f32";
  AFD_REQUIRE(X && sum && outer, "%s: X, sum and outer must not be NULL", name);
  AFD_REQUIRE(workspace, "%s: workspace must not be NULL", name);
  AFD_REQUIRE(n > 0 && D > 0, "%s: n and D must be positive (got %ld, %ld)", name, n, D);
  AFD_REQUIRE(mom_sizes_ok(n, D), "%s: n must be below 2^31, D at most 2^15 and n D at most 2^40 (got n = %ld, D = %ld)", name, n, D);
  AFD_REQUIRE(accumulate == 0 || accumulate == 1, "%s: accumulate must be 0 or 1 (got %d)", name, accumulate);
  AFD_REQUIRE(((uintptr_t)X & 3) == 0, "%s: X must be 4-byte aligned", name);
  AFD_REQUIRE((((uintptr_t)sum | (uintptr_t)outer | (uintptr_t)workspace) & 7) == 0, "%s: sum, outer and workspace must be 8-byte aligned", name);
  const size_t need = afd_feature_moments_workspace_bytes(n, D);
  AFD_REQUIRE(workspace_bytes >= need, "%s: workspace too small: %zu bytes given, afd_feature_moments_workspace_bytes asks for %zu", name,
              workspace_bytes, need);
  const long xb = n * D * 4, sb = D * 8, ob = D * D * 8;
  AFD_REQUIRE(!overlaps(sum, sb, X, xb) && !overlaps(outer, ob, X, xb) && !overlaps(workspace, (long)need, X, xb),
              "%s: sum, outer and workspace must not overlap X", name);
  AFD_REQUIRE(!overlaps(sum, sb, outer, ob) && !overlaps(workspace, (long)need, sum, sb) && !overlaps(workspace, (long)need, outer, ob),
              "%s: sum, outer and workspace must not overlap each other", name);
  const long T = mom_tiles(D), pairs = mom_pairs(D), slabs = mom_slabs(n, D);
  const long per = (n + slabs - 1) / slabs, G = (n + per - 1) / per;           // no slab is empty
  double* ws = static_cast<double*>(workspace);
  double* ws_sum = ws + (size_t)slabs * (size_t)pairs * kTile * kTile;
  hipStream_t stream = as_stream(st);
  hipLaunchKernelGGL(moments_k, dim3((unsigned)(pairs * G)), dim3(kTileThreads), 0, stream, X, n, (int)D, (int)T, per, G, ws, ws_sum);
  hipLaunchKernelGGL(moments_finish_k, dim3((unsigned)pairs), dim3(kTileThreads), 0, stream, ws, ws_sum, (int)D, (int)T, G, accumulate, sum, outer);
  return check_launch(name);
}

size_t afd_poly_mmd_workspace_bytes(long S, long m, long D) {
  if (!mmd_sizes_ok(S, m, D)) return 0;
  return (size_t)S * (size_t)mmd_per_subset(m) * sizeof(double);
}

int afd_poly_mmd_sums_f32(const float* A, long na, const float* B, long nb, long D, const int64_t* ia, const int64_t* ib, long S, long m,
                          int degree, double gamma, double coef0, double* sums, void* workspace, size_t workspace_bytes, afd_stream_t st) {
  const char* name = "afd_poly_mmd_sums_f32";
  AFD_REQUIRE(A && B && ia && ib && sums, "%s: A, B, ia, ib and sums must not be NULL", name);
  AFD_REQUIRE(workspace, "%s: workspace must not be NULL", name);
  AFD_REQUIRE(na > 0 && nb > 0 && D > 0 && S > 0, "%s: na, nb, D and S must be positive (got %ld, %ld, %ld, %ld)", name, na, nb, D, S);
  AFD_REQUIRE(m >= 2, "%s: m must be at least 2 (got %ld)", name, m);
  AFD_REQUIRE(degree >= 1 && degree <= 8, "%s: degree must lie in [1, 8] (got %d)", name, degree);
  AFD_REQUIRE(mmd_sizes_ok(S, m, D), "%s: m must be at most %ld, D below 2^31 and S times the tiles of a subset below 2^31 (got S = %ld, m = %ld, D = %ld)",
              name, kMmdMaxM, S, m, D);
  AFD_REQUIRE(na <= (1L << 40) / D && nb <= (1L << 40) / D, "%s: na D and nb D must be at most 2^40 (got %ld, %ld, D = %ld)", name, na, nb, D);
  AFD_REQUIRE((((uintptr_t)A | (uintptr_t)B) & 3) == 0, "%s: A and B must be 4-byte aligned", name);
  AFD_REQUIRE((((uintptr_t)ia | (uintptr_t)ib | (uintptr_t)sums | (uintptr_t)workspace) & 7) == 0,
              "%s: ia, ib, sums and workspace must be 8-byte aligned", name);
  const size_t need = afd_poly_mmd_workspace_bytes(S, m, D);
  AFD_REQUIRE(workspace_bytes >= need, "%s: workspace too small: %zu bytes given, afd_poly_mmd_workspace_bytes asks for %zu", name,
              workspace_bytes, need);
  const long ub = S * 3 * 8;
  struct { const void* p; long bytes; const char* what; } in[] = {{A, na * D * 4, "A"}, {B, nb * D * 4, "B"}, {ia, S * m * 8, "ia"}, {ib, S * m * 8, "ib"}};
  for (const auto& a : in)
    AFD_REQUIRE(!overlaps(sums, ub, a.p, a.bytes) && !overlaps(workspace, (long)need, a.p, a.bytes), "%s: sums and workspace must not overlap %s",
                name, a.what);
  AFD_REQUIRE(!overlaps(workspace, (long)need, sums, ub), "%s: sums and workspace must not overlap each other", name);
  const long MT = mmd_tiles(m), per_subset = mmd_per_subset(m);
  double* ws = static_cast<double*>(workspace);
  hipStream_t stream = as_stream(st);
  hipLaunchKernelGGL(mmd_k, dim3((unsigned)(S * per_subset)), dim3(kTileThreads), 0, stream, A, na, B, nb, (int)D, ia, ib, (int)m, (int)MT, per_subset,
                     degree, gamma, coef0, ws);
  hipLaunchKernelGGL(mmd_finish_k, dim3((unsigned)(3 * S)), dim3(kWave), 0, stream, ws, (int)MT, per_subset, sums);
  return check_launch(name);
}

}  // extern "C"

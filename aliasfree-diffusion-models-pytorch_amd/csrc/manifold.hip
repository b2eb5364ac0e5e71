// manifold.hip -- the two fp64 contractions behind precision / recall / density / coverage, on the fp64
// matrix pipe (mfma_f64_16x16x4_f64), each with its selection fused behind it so that no distance matrix ever reaches memory:
//   afd_kth_neighbour_f32     per row of (n, D) fp32 features the k-th smallest squared distance to another row: the ball radii
//   afd_ball_membership_f32   per query the number of store rows whose ball holds it, and its nearest store row
// The distance is the Gram form d2(a, b) = max(0, (s_a + s_b) - 2 a.b).  a.b is one chain of MFMAs over k, 4 k per instruction in
// ascending order, from a zero accumulator; s_a = a.a is the SAME chain (the diagonal of a tile of A A^T, mf_norms_k), so
// d2(a, a) = (s + s) - 2 s = 0 exactly, and d2 depends on the two rows and D alone: not on n, on the tile, or on which row is the
// query.  Every product of two widened floats is exact (24 x 24 bits), only the additions round.
// Each call is the small pre-pass mf_norms_k, which leaves the squared norms in the workspace, and two launches: workgroup (stripe,
// segment) of four waves carries a stripe of 64 rows past the 64-row tiles of its segment of the other side and leaves the stripe's
// partial results in the workspace (a row's k smallest distances of the segment; its count and nearest row there), and a second
// kernel folds the segments in index order.  The number of segments depends on the sizes alone.  No atomics, no memset, nothing
// depends on the order in which workgroups run.  The distance tiles are the 64 x 64 tiles of f64_tile.h; operands are widened to fp64
// into LDS as s[k][row], 32 k at a time, rows and k beyond the arrays as zeros, the next round's floats loaded into registers
// while the matrix pipe works on this one.
#include "f64_tile.h"

namespace afd {

// (kTile: the rows of a stripe, and of a tile of the other side)
constexpr int kMfPitch = 65;                       // s[k][row], written k-fastest; also the pitch of the distance tile
constexpr int kMfMaxK = 16;
constexpr int kMfListPitch = kMfMaxK + 1;
constexpr long kMfTarget = 4096;                   // workgroups the second launch aims for, whatever the device
constexpr long kMfMaxSegments = 64;                // (one lane per segment in the fold of the k-th neighbour)
constexpr int kMfSmem = 2 * kTileK * kMfPitch;     // doubles: the two staged operands, and over them the 64 x 65 distance tile
static_assert(kMfSmem >= kTile * kMfPitch, "the distance tile fits over the staged operands");

// The thread's elements of a round: k = tid & 31, rows (tid >> 5) + 8 j of the 64 from row0 (row0 < rows).  One uniform base and
// 32-bit offsets per thread (64 rows of at most 2^15 floats).
__device__ __forceinline__ void mf_fetch(const float* __restrict__ src, long rows, int D, long row0, int d0, int tid, float (&v)[kTilePer]) {
  const int k = tid & 31, r = tid >> 5;
  const long left = rows - row0;
  const int lim = d0 + k < D ? (left < kTile ? (int)left : kTile) : 0;      // the rows of the tile this thread may read
  const float* p = src + (row0 * D + d0);
  const int o = r * D + k, step = 8 * D;
#pragma unroll
  for (int j = 0; j < kTilePer; ++j) v[j] = r + 8 * j < lim ? p[o + j * step] : 0.0f;
}

// ---- squared norms -----------------------------------------------------------------------------------------------------------------
// Workgroup b < ta: rows [64 b, 64 b + 64) of A, else rows [64 (b - ta), ...) of B.  Wave w runs the chain of the cross term on
// rows 16 w .. 16 w + 15 against themselves and keeps the diagonal: row i of the tile is in lane (i & 3) * 16 + i, register i >> 2.
__global__ __launch_bounds__(kTileThreads) void mf_norms_k(const float* __restrict__ A, long na, const float* __restrict__ B, long nb, int D,
                                                         long ta, double* __restrict__ norm_a, double* __restrict__ norm_b) {
  __shared__ double s[kTileK * kMfPitch];
  const int tid = threadIdx.x;
  const TileLane q = tile_lane(tid);
  const bool second = (long)blockIdx.x >= ta;
  const float* src = second ? B : A;
  const long rows = second ? nb : na, row0 = ((long)blockIdx.x - (second ? ta : 0)) * kTile;
  double* out = second ? norm_b : norm_a;
  v4d acc = v4d{0.0, 0.0, 0.0, 0.0};
  float nx[kTilePer];
  mf_fetch(src, rows, D, row0, 0, tid, nx);
  for (int d0 = 0; d0 < D; d0 += kTileK) {
    tile_stage_kfast<kMfPitch>(s, tid, nx);
    __syncthreads();
    if (d0 + kTileK < D) mf_fetch(src, rows, D, row0, d0 + kTileK, tid, nx);
#pragma unroll
    for (int kk = 0; kk < kTileK / 4; ++kk) {
      const double a = s[(4 * kk + q.g4) * kMfPitch + 16 * q.w + q.c16];
      acc = mma_f64(a, a, acc);
    }
    __syncthreads();
  }
  const int r = q.c16 >> 2;
  const double v = r == 0 ? acc[0] : r == 1 ? acc[1] : r == 2 ? acc[2] : acc[3];
  const long row = row0 + 16 * q.w + q.c16;
  if (q.g4 == (q.c16 & 3) && row < rows) out[row] = v;
}

// The 64 x 64 tile of d2 between the stripe from row I of A and the rows from J of B, left in smem[row * 65 + column] (over the
// staged operands).  nx_a / nx_b hold the first round's elements on entry and, on return, those of the tile from next_j (if next_j is
// below j_end, the end of the workgroup's segment).  Ends behind a barrier: the tile is complete.
__device__ __forceinline__ void mf_distance_tile(const float* __restrict__ A, long na, const float* __restrict__ B, long nb, int D, long I, long J,
                                                 long next_j, long j_end, const double* sn_a, const double* sn_b, double* smem, float (&nx_a)[kTilePer],
                                                 float (&nx_b)[kTilePer], int tid) {
  double* sa = smem;
  double* sb = smem + kTileK * kMfPitch;
  const TileLane q = tile_lane(tid);
  v4d acc[2][2];
  tile_zero(acc);
  for (int d0 = 0; d0 < D; d0 += kTileK) {
    tile_stage_kfast<kMfPitch>(sa, tid, nx_a);
    tile_stage_kfast<kMfPitch>(sb, tid, nx_b);
    __syncthreads();
    const bool more = d0 + kTileK < D;
    if (more || next_j < j_end) {
      mf_fetch(A, na, D, I, more ? d0 + kTileK : 0, tid, nx_a);
      mf_fetch(B, nb, D, more ? J : next_j, more ? d0 + kTileK : 0, tid, nx_b);
    }
    tile_round<kMfPitch>(sa, sb, q, acc);
    __syncthreads();                               // every wave is done with the operands: the distance tile goes over them
  }
  tile_for_each(q, acc, [&](int row, int col, double dot) {
    const double d = (sn_a[row] + sn_b[col]) - 2.0 * dot;
    smem[row * kMfPitch + col] = d < 0.0 ? 0.0 : d;          // (a select: a NaN stays a NaN)
  });
  __syncthreads();
}

// ---- the k-th neighbour ------------------------------------------------------------------------------------------------------------
// Workgroup (b, g): rows [64 b, 64 b + 64) of X against rows [g seg, min(n, (g + 1) seg)) of X, seg a multiple of 64.  list[row]
// holds the row's k smallest distances so far, ascending (+inf: an empty slot).  Per tile every thread tests 16 distances of one
// row against the row's current k-th and leaves a bit mask; thread `row` then inserts the few that passed, in column order.  A
// NaN compares false and is no candidate.  The lists go to the workspace as [segment][row][k].
__global__ __launch_bounds__(kTileThreads, 2) void mf_kth_k(const float* __restrict__ X, long n, int D, int k, long seg,
                                                          const double* __restrict__ norms, double* __restrict__ parts) {
  __shared__ double smem[kMfSmem];
  __shared__ double list[kTile * kMfListPitch];
  __shared__ double sn_a[kTile], sn_b[kTile];
  __shared__ unsigned mask[kTileThreads];
  const int tid = threadIdx.x, row = tid & 63, part = tid >> 6;
  const long I = (long)blockIdx.x * kTile, gi = I + row;
  const double inf = __builtin_inf();
  if (tid < kTile) {
#pragma unroll
    for (int t = 0; t < kMfMaxK; ++t) list[tid * kMfListPitch + t] = inf;
    sn_a[tid] = I + tid < n ? norms[I + tid] : 0.0;
  }
  float nx_a[kTilePer], nx_b[kTilePer];
  mf_fetch(X, n, D, I, 0, tid, nx_a);
  const long j_begin = (long)blockIdx.y * seg, j_end = j_begin + seg < n ? j_begin + seg : n;
  mf_fetch(X, n, D, j_begin, 0, tid, nx_b);
  for (long J = j_begin; J < j_end; J += kTile) {
    if (tid < kTile) sn_b[tid] = J + tid < n ? norms[J + tid] : 0.0;   // (read behind the barriers of the tile)
    mf_distance_tile(X, n, X, n, D, I, J, J + kTile, j_end, sn_a, sn_b, smem, nx_a, nx_b, tid);
    const double thr = list[row * kMfListPitch + k - 1];
    unsigned m = 0;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      const long j = J + 16 * part + c;
      const double d = smem[row * kMfPitch + 16 * part + c];
      if (j < n && j != gi && d < thr) m |= 1u << c;
    }
    mask[tid] = m;
    __syncthreads();
    if (tid < kTile) {
      double* mine = list + tid * kMfListPitch;
      for (int p = 0; p < 4; ++p) {
        unsigned mm = mask[p * kTile + tid];
        while (mm) {
          const int c = __builtin_ctz(mm);
          mm &= mm - 1;
          const double d = smem[tid * kMfPitch + 16 * p + c];
          if (d < mine[k - 1]) {
            int pos = k - 1;
            while (pos > 0 && mine[pos - 1] > d) {
              mine[pos] = mine[pos - 1];
              --pos;
            }
            mine[pos] = d;
          }
        }
      }
    }
    __syncthreads();                               // the tile and the masks are free again, the lists are up to date
  }
  if (tid < kTile && gi < n) {
    double* out = parts + ((long)blockIdx.y * n + gi) * k;
    for (int t = 0; t < k; ++t) out[t] = list[tid * kMfListPitch + t];
  }
}

// Wave i: the k-th smallest of row i's S ascending lists of k.  Lane s holds its position in list s; a round takes the smallest
// head (the lowest lane among equal ones moves on), and round k's is the answer; +inf once the candidates have run out.
__global__ __launch_bounds__(kTileThreads) void mf_kth_fold_k(const double* __restrict__ part, long n, int k, int S, double* __restrict__ radius2) {
  const int lane = threadIdx.x & 63;
  const long i = (long)blockIdx.x * (kTileThreads / kWave) + (threadIdx.x >> 6);
  if (i >= n) return;                                // (the whole wave)
  const double inf = __builtin_inf();
  const double* mine = part + ((long)(lane < S ? lane : 0) * n + i) * k;
  int pos = 0;
  double m = inf;
  for (int t = 0; t < k; ++t) {
    const double head = (lane < S && pos < k) ? mine[pos] : inf;
    m = head;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double x = __shfl_xor(m, o, kWave);
      m = x < m ? x : m;
    }
    if (!(m < inf)) break;
    const unsigned long long b = __ballot(head == m);
    if (lane == __builtin_ctzll(b)) ++pos;
  }
  if (lane == 0) radius2[i] = m;
}

// ---- ball membership ---------------------------------------------------------------------------------------------------------------
// Workgroup (b, g): queries [64 b, 64 b + 64) against store rows [g seg, min(nr, (g + 1) seg)).  Thread (row, part) walks columns
// 16 part .. 16 part + 15 of every tile in ascending store index and keeps its count and its nearest row (strictly smaller only:
// the lower index stays); the four parts of a row are joined at the end by (distance, index) and left in the workspace.
__global__ __launch_bounds__(kTileThreads, 2) void mf_ball_k(const float* __restrict__ Q, long nq, const float* __restrict__ R, long nr, int D,
                                                        const double* __restrict__ radius2, const int64_t* __restrict__ exclude,
                                                        const double* __restrict__ norm_q, const double* __restrict__ norm_r, long seg,
                                                        double* __restrict__ part_d, long* __restrict__ part_j, int* __restrict__ part_c) {
  __shared__ double smem[kMfSmem];
  __shared__ double sn_a[kTile], sn_b[kTile], rad[kTile];
  const int tid = threadIdx.x, row = tid & 63, part = tid >> 6;
  const long I = (long)blockIdx.x * kTile, gi = I + row;
  const long ex = (exclude && gi < nq) ? exclude[gi] : -1;
  if (tid < kTile) sn_a[tid] = I + tid < nq ? norm_q[I + tid] : 0.0;
  int cnt = 0;
  long best_j = -1;
  double best = __builtin_inf();
  float nx_a[kTilePer], nx_b[kTilePer];
  mf_fetch(Q, nq, D, I, 0, tid, nx_a);
  const long j_begin = (long)blockIdx.y * seg, j_end = j_begin + seg < nr ? j_begin + seg : nr;
  mf_fetch(R, nr, D, j_begin, 0, tid, nx_b);
  for (long J = j_begin; J < j_end; J += kTile) {
    if (tid < kTile) {                             // (read behind the barriers of the tile)
      sn_b[tid] = J + tid < nr ? norm_r[J + tid] : 0.0;
      rad[tid] = J + tid < nr ? radius2[J + tid] : 0.0;
    }
    mf_distance_tile(Q, nq, R, nr, D, I, J, J + kTile, j_end, sn_a, sn_b, smem, nx_a, nx_b, tid);
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      const int col = 16 * part + c;
      const long j = J + col;
      const double d = smem[row * kMfPitch + col];
      if (j < nr && j != ex) {
        if (d <= rad[col]) ++cnt;                    // false for a NaN on either side
        if (d < best || (best_j < 0 && d == d)) {
          best = d;
          best_j = j;
        }
      }
    }
    __syncthreads();                               // the tile is free again
  }
  double* jd = smem;                                 // the parts' results: [part][row]
  long* jj = reinterpret_cast<long*>(smem + kTileThreads);
  int* jc = reinterpret_cast<int*>(smem + 2 * kTileThreads);
  jd[tid] = best;
  jj[tid] = best_j;
  jc[tid] = cnt;
  __syncthreads();
  if (tid < kTile && gi < nq) {
    for (int p = 1; p < 4; ++p) {
      const double d = jd[p * kTile + tid];
      const long j = jj[p * kTile + tid];
      cnt += jc[p * kTile + tid];
      if (j >= 0 && (best_j < 0 || d < best || (d == best && j < best_j))) {
        best = d;
        best_j = j;
      }
    }
    const long o = (long)blockIdx.y * nq + gi;
    part_d[o] = best;
    part_j[o] = best_j;
    part_c[o] = cnt;
  }
}

// Thread q folds query q's S partial results in segment order: the segments ascend in store index, so on equal distances the
// lower index stays.
__global__ __launch_bounds__(kTileThreads) void mf_ball_fold_k(const double* __restrict__ part_d, const long* __restrict__ part_j,
                                                             const int* __restrict__ part_c, long nq, int S, int* __restrict__ count,
                                                             int64_t* __restrict__ nearest, double* __restrict__ nearest_d2) {
  const long q = (long)blockIdx.x * kTileThreads + threadIdx.x;
  if (q >= nq) return;
  int cnt = 0;
  long best_j = -1;
  double best = __builtin_inf();
  for (int s = 0; s < S; ++s) {
    const long o = (long)s * nq + q, j = part_j[o];
    const double d = part_d[o];
    cnt += part_c[o];
    if (j >= 0 && (best_j < 0 || d < best)) {
      best = d;
      best_j = j;
    }
  }
  if (count) count[q] = cnt;
  if (nearest) {
    nearest[q] = best_j;
    nearest_d2[q] = best;
  }
}

static bool mf_rows_ok(long n, long D) { return n > 0 && D > 0 && n < (1L << 31) && D <= (1L << 15) && D <= (1L << 40) / n; }
static long mf_stripes(long n) { return (n + kTile - 1) / kTile; }
// the store's tiles are cut into segments of `per` tiles each, a number that depends on the two sizes alone; no segment is empty
static long mf_tiles_per_segment(long nq, long nr) {
  const long stripes = mf_stripes(nq), tiles = mf_stripes(nr);
  long S = (kMfTarget + stripes - 1) / stripes;
  S = S > kMfMaxSegments ? kMfMaxSegments : S;
  S = S > tiles ? tiles : S;
  return (tiles + S - 1) / S;
}
static long mf_segments(long nq, long nr) {
  const long per = mf_tiles_per_segment(nq, nr);
  return (mf_stripes(nr) + per - 1) / per;
}

}  // namespace afd
using namespace afd;

extern "C" {

size_t afd_kth_neighbour_workspace_bytes(long n, long D, long k) {
  if (!mf_rows_ok(n, D) || k < 1 || k > kMfMaxK) return 0;
  return ((size_t)n + (size_t)mf_segments(n, n) * (size_t)n * (size_t)k) * sizeof(double);
}

int afd_kth_neighbour_f32(const float* X, long n, long D, long k, double* radius2, void* workspace, size_t workspace_bytes, afd_stream_t st) {
  const char* name = "afd_kth_neighbour_f32";
  AFD_REQUIRE(X && radius2, "%s: X and radius2 must not be NULL", name);
  AFD_REQUIRE(workspace, "%s: workspace must not be NULL", name);
  AFD_REQUIRE(n > 0 && D > 0, "%s: n and D must be positive (got %ld, %ld)", name, n, D);
  AFD_REQUIRE(k >= 1 && k <= kMfMaxK, "%s: k must lie in [1, %d] (got %ld)", name, kMfMaxK, k);
  AFD_REQUIRE(mf_rows_ok(n, D), "%s: n must be below 2^31, D at most 2^15 and n D at most 2^40 (got n = %ld, D = %ld)", name, n, D);
  AFD_REQUIRE(((uintptr_t)X & 3) == 0, "%s: X must be 4-byte aligned", name);
  AFD_REQUIRE((((uintptr_t)radius2 | (uintptr_t)workspace) & 7) == 0, "%s: radius2 and workspace must be 8-byte aligned", name);
  const size_t need = afd_kth_neighbour_workspace_bytes(n, D, k);
  AFD_REQUIRE(workspace_bytes >= need, "%s: workspace too small: %zu bytes given, afd_kth_neighbour_workspace_bytes asks for %zu", name,
              workspace_bytes, need);
  const long xb = n * D * 4, rb = n * 8;
  AFD_REQUIRE(!overlaps(radius2, rb, X, xb) && !overlaps(workspace, (long)need, X, xb), "%s: radius2 and workspace must not overlap X", name);
  AFD_REQUIRE(!overlaps(workspace, (long)need, radius2, rb), "%s: radius2 and workspace must not overlap each other", name);
  double* norms = static_cast<double*>(workspace);
  double* part = norms + n;
  const long T = mf_stripes(n), S = mf_segments(n, n), seg = mf_tiles_per_segment(n, n) * kTile;
  hipStream_t stream = as_stream(st);
  hipLaunchKernelGGL(mf_norms_k, dim3((unsigned)T), dim3(kTileThreads), 0, stream, X, n, X, 0L, (int)D, T, norms, norms);
  hipLaunchKernelGGL(mf_kth_k, dim3((unsigned)T, (unsigned)S), dim3(kTileThreads), 0, stream, X, n, (int)D, (int)k, seg, norms, part);
  hipLaunchKernelGGL(mf_kth_fold_k, dim3((unsigned)((n + 3) / 4)), dim3(kTileThreads), 0, stream, part, n, (int)k, (int)S, radius2);
  return check_launch(name);
}

size_t afd_ball_membership_workspace_bytes(long nq, long nr, long D) {
  if (!mf_rows_ok(nq, D) || !mf_rows_ok(nr, D)) return 0;
  const size_t parts = (size_t)mf_segments(nq, nr) * (size_t)nq;     // a double, an int64 and an int32 each
  return ((size_t)nq + (size_t)nr + 2 * parts + (parts + 1) / 2) * sizeof(double);
}

int afd_ball_membership_f32(const float* Q, long nq, const float* R, long nr, long D, const double* radius2, const int64_t* exclude, int* count,
                            int64_t* nearest, double* nearest_d2, void* workspace, size_t workspace_bytes, afd_stream_t st) {
  const char* name = "afd_ball_membership_f32";
  AFD_REQUIRE(Q && R && radius2, "%s: Q, R and radius2 must not be NULL", name);
  AFD_REQUIRE((nearest != nullptr) == (nearest_d2 != nullptr), "%s: nearest and nearest_d2 go together", name);
  AFD_REQUIRE(count || nearest, "%s: nothing to compute (count, nearest and nearest_d2 are all NULL)", name);
  AFD_REQUIRE(workspace, "%s: workspace must not be NULL", name);
  AFD_REQUIRE(nq > 0 && nr > 0 && D > 0, "%s: nq, nr and D must be positive (got %ld, %ld, %ld)", name, nq, nr, D);
  AFD_REQUIRE(mf_rows_ok(nq, D) && mf_rows_ok(nr, D),
              "%s: nq and nr must be below 2^31, D at most 2^15 and nq D, nr D at most 2^40 (got nq = %ld, nr = %ld, D = %ld)", name, nq, nr, D);
  AFD_REQUIRE((((uintptr_t)Q | (uintptr_t)R) & 3) == 0, "%s: Q and R must be 4-byte aligned", name);
  AFD_REQUIRE(((uintptr_t)count & 3) == 0, "%s: count must be 4-byte aligned", name);
  AFD_REQUIRE((((uintptr_t)radius2 | (uintptr_t)exclude | (uintptr_t)nearest | (uintptr_t)nearest_d2 | (uintptr_t)workspace) & 7) == 0,
              "%s: radius2, exclude, nearest, nearest_d2 and workspace must be 8-byte aligned", name);
  const size_t need = afd_ball_membership_workspace_bytes(nq, nr, D);
  AFD_REQUIRE(workspace_bytes >= need, "%s: workspace too small: %zu bytes given, afd_ball_membership_workspace_bytes asks for %zu", name,
              workspace_bytes, need);
  struct { const void* p; long bytes; const char* what; } in[] = {{Q, nq * D * 4, "Q"}, {R, nr * D * 4, "R"}, {radius2, nr * 8, "radius2"},
                                                                  {exclude, nq * 8, "exclude"}},
      out[] = {{count, nq * 4, "count"}, {nearest, nq * 8, "nearest"}, {nearest_d2, nq * 8, "nearest_d2"}, {workspace, (long)need, "workspace"}};
  for (const auto& o : out)
    for (const auto& a : in)
      AFD_REQUIRE(!o.p || !overlaps(o.p, o.bytes, a.p, a.bytes), "%s: count, nearest, nearest_d2 and workspace must not overlap %s", name, a.what);
  for (int i = 0; i < 4; ++i)
    for (int j = i + 1; j < 4; ++j)
      AFD_REQUIRE(!out[i].p || !overlaps(out[i].p, out[i].bytes, out[j].p, out[j].bytes),
                  "%s: count, nearest, nearest_d2 and workspace must not overlap each other", name);
  const long TQ = mf_stripes(nq), TR = mf_stripes(nr), S = mf_segments(nq, nr), seg = mf_tiles_per_segment(nq, nr) * kTile;
  double* norm_q = static_cast<double*>(workspace);
  double* norm_r = norm_q + nq;
  double* part_d = norm_r + nr;
  long* part_j = reinterpret_cast<long*>(part_d + S * nq);
  int* part_c = reinterpret_cast<int*>(part_j + S * nq);
  hipStream_t stream = as_stream(st);
  hipLaunchKernelGGL(mf_norms_k, dim3((unsigned)(TQ + TR)), dim3(kTileThreads), 0, stream, Q, nq, R, nr, (int)D, TQ, norm_q, norm_r);
  hipLaunchKernelGGL(mf_ball_k, dim3((unsigned)TQ, (unsigned)S), dim3(kTileThreads), 0, stream, Q, nq, R, nr, (int)D, radius2, exclude, norm_q, norm_r,
                     seg, part_d, part_j, part_c);
  hipLaunchKernelGGL(mf_ball_fold_k, dim3((unsigned)((nq + kTileThreads - 1) / kTileThreads)), dim3(kTileThreads), 0, stream, part_d, part_j, part_c, nq,
                     (int)S, count, nearest, nearest_d2);
  return check_launch(name);
}

}  // extern "C"

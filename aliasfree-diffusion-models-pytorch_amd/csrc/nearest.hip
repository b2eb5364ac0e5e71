// nearest.hip -- nearest-store-row search: for each of n query rows, the k rows of an (N, D) store of smallest squared L2 distance,
// ascending, ties to the lower store index.  DESIGN.md section 6o has the semantics, the integer bounds and the tiling.
//
// u8: d^2 = sum a'^2 + sum b'^2 - 2 sum a'b' with a' = a - 128 as int8 (byte ^ 0x80), the cross term on the i8 matrix pipe
// (mfma_i32_16x16x64_i8, int32 accumulators), the norms from sdot4 on the fragments already loaded: exact.
// f32: sum ((double)a - (double)b)^2 in fp64, rounded once to fp32, on the vector pipe.
// Selection: (distance bits << 32 | store index) is one unsigned key per candidate, every key unique, the k smallest are the
// answer.  A workgroup owns a chunk of store rows and leaves its k smallest keys per query, ascending, in the workspace; nn_merge_k
// merges the chunks' lists.  Nothing depends on the order in which workgroups or lanes run.
#include "common.h"

namespace afd {

typedef int v4i __attribute__((ext_vector_type(4)));

constexpr uint64_t kNoKey = ~0ull;                 // "no candidate": above every real key (a store index is below 2^31)
constexpr uint32_t kNaNBits = 0x7fc00000u, kInfBits = 0x7f800000u;
constexpr int kMaxK = 16;
constexpr long kMaxChunks = 512;                   // workgroups of a search launch: two per CU
constexpr long kMaxD8 = 32768;                     // D 255^2 < 2^31 and D 2^14 <= 2^29: int32 holds all three sums

// ---- selection ---------------------------------------------------------------------------------------------------------------------
// 16 consecutive lanes (a "row" of the wave) own one query.  Its candidates are CPL columns per lane of `trow` (distance bits of
// store rows r0 + column) and, from the second tile of the chunk on, the k keys this workgroup left in wsq.  k rounds, each the
// smallest key above the round before: keys are unique, so round t is rank t.  Every lane of the workgroup runs every round
// (k is uniform); `active` only masks what is read and written.
template <int CPL>
__device__ __forceinline__ void select_row(const uint32_t* trow, long r0, long N, long ex, bool active, bool first, uint64_t* wsq,
                                           int k, int r) {
  uint64_t cand[CPL + 1];
#pragma unroll
  for (int i = 0; i < CPL; ++i) {
    const int col = r + 16 * i;
    const long j = r0 + col;
    cand[i] = (active && j < N && j != ex) ? ((uint64_t)trow[col] << 32 | (uint64_t)j) : kNoKey;
  }
  cand[CPL] = (active && !first && r < k) ? wsq[r] : kNoKey;
  uint64_t last = 0, mine = kNoKey;
  for (int t = 0; t < k; ++t) {
    uint64_t b = kNoKey;
#pragma unroll
    for (int i = 0; i <= CPL; ++i) {
      const uint64_t c = cand[i];
      if ((t == 0 || c > last) && c < b) b = c;
    }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
      const uint64_t x = __shfl_xor(b, o, 16);
      b = x < b ? x : b;
    }
    if (r == t) mine = b;
    last = b;                                      // (kNoKey once the candidates run out: nothing is above it)
  }
  if (active && r < k) wsq[r] = mine;
}

// ---- u8 on the matrix pipe ---------------------------------------------------------------------------------------------------------
constexpr int kQT = 128, kRT = 128;                // queries and store rows of one tile: 8 x (4 waves x 2) MFMA tiles of 16 x 16
constexpr int kSlab = 256, kSlabPitch = kSlab + 16;    // K bytes of the queries held in LDS at a time; +16: rows 17 units apart
constexpr int kTilePitch = kRT + 1;
constexpr int kSmem8 = kQT * kTilePitch * 4;       // the distance tile (66 048 B) shares LDS with the query slab (34 816 B)

// 16 bytes of `row` from k0 as int8 values a - 128; bytes at k >= D are 0.  FAST: D % 16 == 0 and a 16-byte aligned row.
template <bool FAST>
__device__ __forceinline__ v4i load16_i8(const uint8_t* __restrict__ row, long k0, long D) {
  if (FAST) {
    if (k0 >= D) return v4i{0, 0, 0, 0};
    const uint4 v = *reinterpret_cast<const uint4*>(row + k0);
    return v4i{(int)(v.x ^ 0x80808080u), (int)(v.y ^ 0x80808080u), (int)(v.z ^ 0x80808080u), (int)(v.w ^ 0x80808080u)};
  }
  uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int j = 0; j < 16; ++j)
    if (k0 + j < D) w[j >> 2] |= (uint32_t)(row[k0 + j] ^ 0x80u) << (8 * (j & 3));
  return v4i{(int)w[0], (int)w[1], (int)w[2], (int)w[3]};
}

__device__ __forceinline__ int dot16(v4i v, int acc) {
  acc = __builtin_amdgcn_sdot4(v.x, v.x, acc, false);
  acc = __builtin_amdgcn_sdot4(v.y, v.y, acc, false);
  acc = __builtin_amdgcn_sdot4(v.z, v.z, acc, false);
  return __builtin_amdgcn_sdot4(v.w, v.w, acc, false);
}

// The MFMAs of one K slab: B fragments b (registers), A fragments from the slab in LDS.  FULL: all 4 K steps and all 8 row tiles,
// straight-line code; otherwise the first ksteps and mt of them (both uniform over the workgroup).
template <bool FULL>
__device__ __forceinline__ void slab_mma(const uint8_t* slab, const v4i (&b)[kSlab / 64][2], v4i (&acc)[8][2], int (&na)[8], int (&nb)[2],
                                         int ksteps, int mt, int c16, int g) {
#pragma unroll
  for (int ks = 0; ks < kSlab / 64; ++ks) {
    if (FULL || ks < ksteps) {
      nb[0] = dot16(b[ks][0], nb[0]);
      nb[1] = dot16(b[ks][1], nb[1]);
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        if (FULL || m < mt) {
          const v4i a = *reinterpret_cast<const v4i*>(slab + (16 * m + c16) * kSlabPitch + 64 * ks + 16 * g);
          na[m] = dot16(a, na[m]);
          acc[m][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b[ks][0], acc[m][0], 0, 0, 0);
          acc[m][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b[ks][1], acc[m][1], 0, 0, 0);
        }
      }
    }
  }
}

// Workgroup (c, y): store rows [c chunk, min(N, (c + 1) chunk)), chunk a multiple of kRT, in tiles of kRT rows; for each tile,
// every tile of kQT queries among queries [y qper, min(n, (y + 1) qper)), qper a multiple of kQT.
// Queries are the rows of A, store rows the columns of B (B[k][j] = data[j][k]), both K-contiguous: lane l holds bytes
// 16 (l >> 4) .. + 15 of the 64-byte K step of row / column l & 15 in BOTH fragments, so whatever order the instruction gives the
// 64 products, each k meets itself.  C: column l & 15, row 4 (l >> 4) + reg.
// Wave w: columns 32 w .. + 31 of the tile (two B fragments from global memory), all 8 row tiles (A fragments from LDS).
template <bool FAST>
__global__ __launch_bounds__(256, 2) void nn_u8_k(const uint8_t* __restrict__ data, long N, long D, const uint8_t* __restrict__ queries,
                                                  long n, const int64_t* __restrict__ exclude, int k, long chunk, long qper, uint64_t* ws) {
  __shared__ uint4 smem[kSmem8 / 16];
  uint8_t* slab = reinterpret_cast<uint8_t*>(smem);
  uint32_t* tile = reinterpret_cast<uint32_t*>(smem);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c16 = lane & 15, g = lane >> 4;
  const long row_begin = blockIdx.x * chunk, row_end = row_begin + chunk < N ? row_begin + chunk : N;
  const long q_begin = blockIdx.y * qper, q_end = q_begin + qper < n ? q_begin + qper : n;
  for (long r0 = row_begin; r0 < row_end; r0 += kRT) {
    const uint8_t* brow[2];
    bool bok[2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const long j = r0 + 32 * w + 16 * nt + c16;
      bok[nt] = j < N;
      brow[nt] = data + (bok[nt] ? j : 0) * D;
    }
    for (long q0 = q_begin; q0 < q_end; q0 += kQT) {
      const int mt = n - q0 >= kQT ? kQT / 16 : (int)((n - q0 + 15) / 16);      // row tiles that hold a query
      v4i acc[8][2];
      int na[8], nb[2] = {0, 0};
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        na[m] = 0;
        acc[m][0] = acc[m][1] = v4i{0, 0, 0, 0};
      }
      for (long s0 = 0; s0 < D; s0 += kSlab) {
        // the slab's B fragments first: their latency passes behind the fill of the slab and its two barriers
        const int ksteps = D - s0 >= kSlab ? kSlab / 64 : (int)((D - s0 + 63) / 64);
        v4i b[kSlab / 64][2];
#pragma unroll
        for (int ks = 0; ks < kSlab / 64; ++ks) {
#pragma unroll
          for (int nt = 0; nt < 2; ++nt)
            b[ks][nt] = (bok[nt] && ks < ksteps) ? load16_i8<FAST>(brow[nt], s0 + 64 * ks + 16 * g, D) : v4i{0, 0, 0, 0};
        }
        __syncthreads();                             // the slab (or the distance tile under it) is no longer read
        for (int u = tid; u < mt * 16 * (kSlab / 16); u += 256) {
          const int row = u >> 4, cu = u & 15;
          const long q = q0 + row;
          const v4i v = q < n ? load16_i8<FAST>(queries + q * D, s0 + 16 * cu, D) : v4i{0, 0, 0, 0};
          *reinterpret_cast<v4i*>(slab + row * kSlabPitch + 16 * cu) = v;
        }
        __syncthreads();
        if (ksteps == kSlab / 64 && mt == kQT / 16) slab_mma<true>(slab, b, acc, na, nb, ksteps, mt, c16, g);
        else slab_mma<false>(slab, b, acc, na, nb, ksteps, mt, c16, g);
      }
      // the norms: each lane summed its quarter of every K step; lanes l, l ^ 16, l ^ 32, l ^ 48 share a row / column
#pragma unroll
      for (int o = 16; o < 64; o <<= 1) {
#pragma unroll
        for (int m = 0; m < 8; ++m) na[m] += __shfl_xor(na[m], o, kWave);
        nb[0] += __shfl_xor(nb[0], o, kWave);
        nb[1] += __shfl_xor(nb[1], o, kWave);
      }
      __syncthreads();                               // every wave is done with the slab: the distance tile goes over it
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        if (m < mt) {
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            const uint32_t naq = (uint32_t)__shfl(na[m], 4 * g + reg, kWave);      // the norm of row 4 g + reg of this row tile
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)       // below 2^32 as a true value, so the wrap-around arithmetic is exact
              tile[(16 * m + 4 * g + reg) * kTilePitch + 32 * w + 16 * nt + c16] = naq + (uint32_t)nb[nt] - 2u * (uint32_t)acc[m][nt][reg];
          }
        }
      }
      __syncthreads();
      for (int p = 0; p < mt; ++p) {
        const int ql = 16 * p + (tid >> 4);
        const long q = q0 + ql;
        const bool active = q < n;
        const long ex = (active && exclude) ? exclude[q] : -1;
        select_row<kRT / 16>(tile + ql * kTilePitch, r0, N, ex, active, r0 == row_begin, ws + ((long)blockIdx.x * n + (active ? q : 0)) * k, k,
                             tid & 15);
      }
    }
  }
}

// ---- f32 on the vector pipe --------------------------------------------------------------------------------------------------------
constexpr int kQTF = 16, kRTF = 256, kSlabF = 32;  // thread t: store row r0 + t against 16 queries, 32 elements of K in LDS at a time

__global__ __launch_bounds__(256) void nn_f32_k(const float* __restrict__ data, long N, long D, const float* __restrict__ queries, long n,
                                                const int64_t* __restrict__ exclude, int k, long chunk, long qper, uint64_t* ws) {
  __shared__ float sd[kRTF * (kSlabF + 1)];
  __shared__ double sq[kQTF * kSlabF];
  __shared__ uint32_t tile[kQTF * (kRTF + 1)];
  const int tid = threadIdx.x;
  const long row_begin = blockIdx.x * chunk, row_end = row_begin + chunk < N ? row_begin + chunk : N;
  const long q_begin = blockIdx.y * qper, q_end = q_begin + qper < n ? q_begin + qper : n;
  for (long r0 = row_begin; r0 < row_end; r0 += kRTF) {
    for (long q0 = q_begin; q0 < q_end; q0 += kQTF) {
      double acc[kQTF];
#pragma unroll
      for (int i = 0; i < kQTF; ++i) acc[i] = 0.0;
      for (long s0 = 0; s0 < D; s0 += kSlabF) {
        __syncthreads();
        for (int u = tid; u < kRTF * kSlabF; u += 256) {
          const int row = u >> 5, c = u & 31;
          const long j = r0 + row, kk = s0 + c;
          sd[row * (kSlabF + 1) + c] = (j < N && kk < D) ? data[j * D + kk] : 0.f;
        }
        for (int u = tid; u < kQTF * kSlabF; u += 256) {
          const int row = u >> 5, c = u & 31;
          const long q = q0 + row, kk = s0 + c;
          sq[row * kSlabF + c] = (q < n && kk < D) ? (double)queries[q * D + kk] : 0.0;
        }
        __syncthreads();
        const int kn = D - s0 >= kSlabF ? kSlabF : (int)(D - s0);
        for (int c = 0; c < kn; ++c) {
          const double b = (double)sd[tid * (kSlabF + 1) + c];
#pragma unroll
          for (int i = 0; i < kQTF; ++i) {
            const double d = b - sq[i * kSlabF + c];
            acc[i] = fma(d, d, acc[i]);
          }
        }
      }
#pragma unroll
      for (int i = 0; i < kQTF; ++i) {
        const float f = (float)acc[i];             // the one rounding
        tile[i * (kRTF + 1) + tid] = f != f ? kNaNBits : __float_as_uint(f);
      }
      __syncthreads();
      const int ql = tid >> 4;
      const long q = q0 + ql;
      const bool active = q < n;
      const long ex = (active && exclude) ? exclude[q] : -1;
      select_row<kRTF / 16>(tile + ql * (kRTF + 1), r0, N, ex, active, r0 == row_begin, ws + ((long)blockIdx.x * n + (active ? q : 0)) * k, k,
                            tid & 15);
    }
  }
}

// ---- merge -------------------------------------------------------------------------------------------------------------------------
// One workgroup per query.  The G lists of k keys the search workgroups left are each ascending, so the k smallest of all are a
// G-way merge: the lists go to LDS in one coalesced pass, thread c holds the position in lists c and c + 256, a round is the
// workgroup's minimum over the lists' heads, and the list that held it (keys are unique) moves on.
constexpr int kMergeThreads = 256;
static_assert(kMaxChunks <= 2 * kMergeThreads && kMaxChunks * kMaxK * 8 <= 64 * 1024, "two lists per thread, all lists in LDS");

template <bool F32>
__global__ __launch_bounds__(kMergeThreads) void nn_merge_k(const uint64_t* __restrict__ ws, int G, long n, int k,
                                                           int64_t* __restrict__ idx, void* __restrict__ dist) {
  __shared__ uint64_t keys[kMaxChunks * kMaxK];
  __shared__ uint64_t red[2][kMergeThreads / kWave];
  const long q = blockIdx.x;
  const int tid = threadIdx.x;
  for (int u = tid; u < G * k; u += kMergeThreads) {
    const int c = u / k, i = u - c * k;
    keys[u] = ws[((long)c * n + q) * k + i];
  }
  __syncthreads();
  int pos[2] = {0, 0};
  for (int t = 0; t < k; ++t) {
    uint64_t head[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int c = tid + j * kMergeThreads;
      head[j] = (c < G && pos[j] < k) ? keys[c * k + pos[j]] : kNoKey;
    }
    uint64_t b = head[0] < head[1] ? head[0] : head[1];
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const uint64_t x = __shfl_xor(b, o, kWave);
      b = x < b ? x : b;
    }
    if ((tid & (kWave - 1)) == 0) red[t & 1][tid / kWave] = b;
    __syncthreads();                               // (red is double-buffered: one barrier per round)
#pragma unroll
    for (int wv = 0; wv < kMergeThreads / kWave; ++wv) b = red[t & 1][wv] < b ? red[t & 1][wv] : b;
    const bool none = b == kNoKey;
    if (!none) {
      if (head[0] == b) ++pos[0];
      if (head[1] == b) ++pos[1];
    }
    if (tid == 0) {
      idx[q * k + t] = none ? -1 : (int64_t)(b & 0xffffffffull);
      if (F32) static_cast<uint32_t*>(dist)[q * k + t] = none ? kInfBits : (uint32_t)(b >> 32);
      else static_cast<int64_t*>(dist)[q * k + t] = none ? -1 : (int64_t)(b >> 32);
    }
  }
}

static long chunk_rows(long N, long tile) {
  const long per = (N + kMaxChunks - 1) / kMaxChunks;
  return (per + tile - 1) / tile * tile;
}
static long n_chunks(long N, bool f32) {
  const long chunk = chunk_rows(N, f32 ? kRTF : kRT);
  return (N + chunk - 1) / chunk;
}
static bool sizes_ok(long N, long D, long n, long k) {
  return N > 0 && D > 0 && n > 0 && k >= 1 && k <= kMaxK && N < (1L << 31) && n < (1L << 31) && D <= (1L << 40) / N && D <= (1L << 40) / n;
}

}  // namespace afd
using namespace afd;

template <bool F32>
static int launch_nn_search(const char* name, const void* data, long N, long D, const void* queries, long n, const int64_t* exclude, long k,
                            int64_t* idx, void* dist, void* workspace, size_t workspace_bytes, hipStream_t st) {
  AFD_REQUIRE(data, "%s: data must not be NULL", name);
  AFD_REQUIRE(queries, "%s: queries must not be NULL", name);
  AFD_REQUIRE(idx, "%s: idx must not be NULL", name);
  AFD_REQUIRE(dist, "%s: dist must not be NULL", name);
  AFD_REQUIRE(workspace, "%s: workspace must not be NULL", name);
  AFD_REQUIRE(N > 0 && D > 0 && n > 0, "%s: N, D and n must be positive (got %ld, %ld, %ld)", name, N, D, n);
  AFD_REQUIRE(k >= 1 && k <= kMaxK, "%s: k must lie in [1, %d] (got %ld)", name, kMaxK, k);
  AFD_REQUIRE(F32 || D <= kMaxD8, "%s: D must be at most %ld for a uint8 store, so that int32 holds every sum (got %ld)", name, kMaxD8, D);
  AFD_REQUIRE(sizes_ok(N, D, n, k), "%s: N and n must be below 2^31 and N D, n D at most 2^40 (got N = %ld, D = %ld, n = %ld)", name, N, D, n);
  const long esz = F32 ? 4 : 1, dsz = F32 ? 4 : 8;
  AFD_REQUIRE(((uintptr_t)idx & 7) == 0, "%s: idx must be 8-byte aligned", name);
  AFD_REQUIRE(((uintptr_t)dist & (dsz - 1)) == 0, "%s: dist must be %ld-byte aligned", name, dsz);
  AFD_REQUIRE(((uintptr_t)exclude & 7) == 0, "%s: exclude must be 8-byte aligned", name);
  AFD_REQUIRE(((uintptr_t)workspace & 7) == 0, "%s: workspace must be 8-byte aligned", name);
  AFD_REQUIRE(!F32 || (((uintptr_t)data & 3) == 0 && ((uintptr_t)queries & 3) == 0), "%s: data and queries must be 4-byte aligned", name);
  const size_t need = afd_nn_search_workspace_bytes(N, D, n, k, F32 ? 1 : 0);
  AFD_REQUIRE(workspace_bytes >= need, "%s: workspace too small: %zu bytes given, afd_nn_search_workspace_bytes asks for %zu", name,
              workspace_bytes, need);
  const long ob = n * k * 8, db = n * k * dsz;
  struct { const void* p; long bytes; const char* what; } in[] = {{data, N * D * esz, "data"}, {queries, n * D * esz, "queries"},
                                                                  {exclude, n * 8, "exclude"}};
  for (const auto& a : in)
    AFD_REQUIRE(!overlaps(idx, ob, a.p, a.bytes) && !overlaps(dist, db, a.p, a.bytes) && !overlaps(workspace, (long)need, a.p, a.bytes),
                "%s: idx, dist and workspace must not overlap %s", name, a.what);
  AFD_REQUIRE(!overlaps(idx, ob, dist, db) && !overlaps(idx, ob, workspace, (long)need) && !overlaps(dist, db, workspace, (long)need),
              "%s: idx, dist and workspace must not overlap each other", name);
  const long chunk = chunk_rows(N, F32 ? kRTF : kRT), G = n_chunks(N, F32);
  // a store of few chunks leaves CUs idle: the query tiles are then split over blockIdx.y (the store is read once per split, from
  // the caches), up to kMaxChunks workgroups in all
  const long qt = F32 ? kQTF : kQT, qtiles = (n + qt - 1) / qt, want = kMaxChunks / G > 1 ? kMaxChunks / G : 1;
  const long per = (qtiles + want - 1) / want, gy = (qtiles + per - 1) / per, qper = per * qt;
  uint64_t* ws = static_cast<uint64_t*>(workspace);
  if (F32) {
    hipLaunchKernelGGL(nn_f32_k, dim3((unsigned)G, (unsigned)gy), dim3(256), 0, st, static_cast<const float*>(data), N, D,
                       static_cast<const float*>(queries), n, exclude, (int)k, chunk, qper, ws);
  } else {
    const uint8_t* d8 = static_cast<const uint8_t*>(data);
    const uint8_t* q8 = static_cast<const uint8_t*>(queries);
    if (D % 16 == 0 && aligned16(data) && aligned16(queries))          // then every row starts 16-byte aligned
      hipLaunchKernelGGL(nn_u8_k<true>, dim3((unsigned)G, (unsigned)gy), dim3(256), 0, st, d8, N, D, q8, n, exclude, (int)k, chunk, qper, ws);
    else
      hipLaunchKernelGGL(nn_u8_k<false>, dim3((unsigned)G, (unsigned)gy), dim3(256), 0, st, d8, N, D, q8, n, exclude, (int)k, chunk, qper, ws);
  }
  hipLaunchKernelGGL(nn_merge_k<F32>, dim3((unsigned)n), dim3(kMergeThreads), 0, st, ws, (int)G, n, (int)k, idx, dist);
  return check_launch(name);
}

extern "C" {

size_t afd_nn_search_workspace_bytes(long N, long D, long n, long k, int f32) {
  if (!sizes_ok(N, D, n, k)) return 0;
  return (size_t)n_chunks(N, f32 != 0) * (size_t)n * (size_t)k * sizeof(uint64_t);
}

int afd_nn_search_u8(const uint8_t* data, long N, long D, const uint8_t* queries, long n, const int64_t* exclude, long k, int64_t* idx,
                     int64_t* dist, void* workspace, size_t workspace_bytes, afd_stream_t st) {
  return launch_nn_search<false>("afd_nn_search_u8", data, N, D, queries, n, exclude, k, idx, dist, workspace, workspace_bytes, as_stream(st));
}

int afd_nn_search_f32(const float* data, long N, long D, const float* queries, long n, const int64_t* exclude, long k, int64_t* idx,
                      float* dist, void* workspace, size_t workspace_bytes, afd_stream_t st) {
  return launch_nn_search<true>("afd_nn_search_f32", data, N, D, queries, n, exclude, k, idx, dist, workspace, workspace_bytes, as_stream(st));
}

}  // extern "C"

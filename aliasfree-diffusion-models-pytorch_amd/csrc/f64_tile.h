// f64_tile.h -- the fp64 matrix-pipe building blocks that fidelity.hip, manifold.hip and spectrum.hip share (DESIGN.md section
// 6u): the MFMA wrapper with its fragment layout, and the 64 x 64 output tile of a workgroup of four waves, each wave a 32 x 32
// quadrant as 2 x 2 MFMA tiles, over operands staged in LDS as s[k][row], 32 k at a time.
#pragma once
#include "common.h"

namespace afd {

typedef double v4d __attribute__((ext_vector_type(4)));

// Fragments of mfma_f64_16x16x4_f64: lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][column l & 15]; result register r of
// lane l is D[row (l >> 4) + 4 r][column l & 15].
__device__ __forceinline__ v4d mma_f64(double a, double b, v4d c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

constexpr int kTile = 64;                          // output tile side
constexpr int kTileThreads = 256;                  // 4 waves, a 32 x 32 quadrant each
constexpr int kTileK = 32;                         // k staged per round
constexpr int kTilePer = kTile * kTileK / kTileThreads;      // elements of one staged operand per thread
static_assert(kTile == 64, "a tile is 2 x 2 quadrants of 2 x 2 MFMA tiles of 16 x 16");
static_assert(kTileThreads == 4 * kWave, "one wave per quadrant");
static_assert(kTileK == 32 && kTileK % 4 == 0, "a round is whole MFMAs of 4 k; a thread stages k = tid & 31");
static_assert(kTilePer == 8, "a thread stages rows (tid >> 5) + 8 j of the 64");

// A lane's place in the tile: fragment column c16 and k group g4, its wave w (scalar: branches on it are taken by whole waves),
// and the wave's quadrant, which starts at row ra of sa and row cb of sb.
struct TileLane {
  int c16, g4, w, ra, cb;
};

__device__ __forceinline__ TileLane tile_lane(int tid) {
  const int lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  return {lane & 15, lane >> 4, w, 32 * (w >> 1), 32 * (w & 1)};
}

// acc[a][b] is the 16 x 16 tile at (ra + 16 a, cb + 16 b) of the 64 x 64.
__device__ __forceinline__ void tile_zero(v4d (&acc)[2][2]) {
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = v4d{0.0, 0.0, 0.0, 0.0};
}

// One round: acc += sa^T sb over the 32 staged k, in ascending k.  sa / sb: the staged operands as s[k][row] at pitch P.
template <int P>
__device__ __forceinline__ void tile_round(const double* sa, const double* sb, const TileLane& q, v4d (&acc)[2][2]) {
#pragma unroll
  for (int kk = 0; kk < kTileK / 4; ++kk) {
    const int o = (4 * kk + q.g4) * P + q.c16;
    const double a0 = sa[o + q.ra], a1 = sa[o + q.ra + 16], b0 = sb[o + q.cb], b1 = sb[o + q.cb + 16];
    acc[0][0] = mma_f64(a0, b0, acc[0][0]);
    acc[0][1] = mma_f64(a0, b1, acc[0][1]);
    acc[1][0] = mma_f64(a1, b0, acc[1][0]);
    acc[1][1] = mma_f64(a1, b1, acc[1][1]);
  }
}

// Stages the thread's elements of a round, k = tid & 31 of rows (tid >> 5) + 8 j, widened to fp64: written k-fastest (32
// consecutive k of one row), so an odd pitch P gives 32 distinct bank pairs.
template <int P>
__device__ __forceinline__ void tile_stage_kfast(double* s, int tid, const float (&v)[kTilePer]) {
  const int k = tid & 31;
#pragma unroll
  for (int j = 0; j < kTilePer; ++j) s[k * P + (tid >> 5) + 8 * j] = (double)v[j];
}

// f(row, column, value) for the lane's 16 elements of the tile, (a, b, r) in ascending order with r fastest: a sum taken in f
// has that order.  Fully unrolled and inlined, so acc is only ever indexed by constants and stays in registers.
template <class F>
__device__ __forceinline__ void tile_for_each(const TileLane& q, const v4d (&acc)[2][2], F&& f) {
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) f(q.ra + 16 * a + q.g4 + 4 * r, q.cb + 16 * b + q.c16, acc[a][b][r]);
}

}  // namespace afd

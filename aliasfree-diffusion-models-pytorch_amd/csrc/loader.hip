// loader.hip -- batch assembly for a data set that lives in device memory: gather B images by index out of an (N, C, H, W) store,
// mirror the flagged rows left-right, turn uint8 pixels into the normalised floats of the host loader through a (C, 256) table
// built on the host, and gather the labels.  One launch per batch.  DESIGN.md section 6n has the semantics and the layout choices.
//
// No arithmetic touches a pixel: the u8 form is a table lookup, the f32 form moves 32-bit words (NaN payloads, infinities and
// -0.0 survive).  An index outside [0, N) reads nothing: the row becomes quiet NaN and its label INT64_MIN.
#include "common.h"

namespace afd {

constexpr uint32_t kQuietNaN = 0x7fc00000u;
constexpr int kVecThreads = 64, kScalarThreads = 256;      // one wave covers a 32 x 32 u8 plane's 64 chunks
constexpr int kMaxPlaneBlocks = 1024;                      // workgroups per plane (blockIdx.y), the rest is a stride loop

__device__ __forceinline__ uint32_t bswap32(uint32_t v) { return __builtin_bswap32(v); }

// Workgroup (p, k): plane p = b * C + c of the output, and the items k * NT + tid, + gridDim.y * NT, ... of that plane.
// An item is one output element (VEC = false) or 16 source bytes (VEC = true: 16 u8 pixels -> four float4 stores, or 4 floats ->
// one).  VEC needs a row of a multiple of 16 source bytes and 16-byte aligned data and x (the launcher checks), so a chunk never
// crosses a row and a mirrored row is the mirrored chunk with its elements reversed in registers.
// U8: the plane's channel of the table, 256 floats, is copied to LDS first -- every pixel is a lookup at a data-dependent
// address, which LDS serves per bank and the vector cache per line.
template <bool U8, bool VEC, int NT>
__global__ __launch_bounds__(NT) void batch_gather_k(const void* __restrict__ data_, long N, long C, long H, long W,
                                                     const int64_t* __restrict__ idx, const uint8_t* __restrict__ flip,
                                                     const float* __restrict__ table, uint32_t* __restrict__ x,
                                                     const int64_t* __restrict__ labels, int64_t* __restrict__ y) {
  __shared__ float tab[256];
  const long p = blockIdx.x, b = p / C, c = p - b * C;
  const long i = idx[b];
  const bool ok = i >= 0 && i < N;
  const bool mirror = flip && flip[b] != 0;
  const long plane = H * W;
  if (U8 && ok) {
    for (int k = threadIdx.x; k < 256; k += NT) tab[k] = table[c * 256 + k];
    __syncthreads();                                  // (ok is uniform over the workgroup)
  }
  if (y && c == 0 && blockIdx.y == 0 && threadIdx.x == 0) y[b] = ok ? labels[i] : INT64_MIN;
  uint32_t* __restrict__ dst = x + p * plane;
  const long src0 = ok ? (i * C + c) * plane : 0;
  if (VEC) {
    constexpr int E = U8 ? 16 : 4;                    // elements per chunk
    const long per_row = W / E, n = plane / E;
    for (long q = blockIdx.y * (long)NT + threadIdx.x; q < n; q += (long)gridDim.y * NT) {
      uint4* o = reinterpret_cast<uint4*>(dst + q * E);
      if (!ok) {
        const uint4 nan4 = make_uint4(kQuietNaN, kQuietNaN, kQuietNaN, kQuietNaN);
#pragma unroll
        for (int k = 0; k < E / 4; ++k) o[k] = nan4;
        continue;
      }
      long s = q;
      if (mirror) {
        const long h = q / per_row, j = q - h * per_row;
        s = h * per_row + (per_row - 1 - j);
      }
      uint4 v;
      if (U8) v = *reinterpret_cast<const uint4*>(static_cast<const uint8_t*>(data_) + src0 + s * 16);
      else v = *reinterpret_cast<const uint4*>(static_cast<const uint32_t*>(data_) + src0 + s * 4);
      if (mirror) {
        if (U8) v = make_uint4(bswap32(v.w), bswap32(v.z), bswap32(v.y), bswap32(v.x));
        else v = make_uint4(v.w, v.z, v.y, v.x);
      }
      if (U8) {
        const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint32_t u = w4[k];
          o[k] = make_uint4(__float_as_uint(tab[u & 255u]), __float_as_uint(tab[(u >> 8) & 255u]),
                            __float_as_uint(tab[(u >> 16) & 255u]), __float_as_uint(tab[u >> 24]));
        }
      } else {
        o[0] = v;
      }
    }
  } else {
    for (long e = blockIdx.y * (long)NT + threadIdx.x; e < plane; e += (long)gridDim.y * NT) {
      if (!ok) {
        dst[e] = kQuietNaN;
        continue;
      }
      long s = e;
      if (mirror) {
        const long h = e / W, w = e - h * W;
        s = h * W + (W - 1 - w);
      }
      if (U8) dst[e] = __float_as_uint(tab[static_cast<const uint8_t*>(data_)[src0 + s]]);
      else dst[e] = static_cast<const uint32_t*>(data_)[src0 + s];
    }
  }
}

}  // namespace afd
using namespace afd;

template <bool U8>
static int launch_batch_gather(const char* name, const void* data, long N, long C, long H, long W, const int64_t* idx,
                               const uint8_t* flip, const float* table, float* x, const int64_t* labels, int64_t* y, long B,
                               hipStream_t st) {
  AFD_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0 && B > 0, "%s: N, C, H, W and B must be positive (got %ld, %ld, %ld, %ld, %ld)", name, N,
              C, H, W, B);
  AFD_REQUIRE((labels == nullptr) == (y == nullptr), "%s: labels and y go together (both NULL, or neither)", name);
  AFD_REQUIRE(C <= 0x7fffffffL / B, "%s: at most 2^31 - 1 output planes per call (got B = %ld, C = %ld)", name, B, C);
  AFD_REQUIRE(H <= (1L << 40) / W && C <= (1L << 40) / (H * W) && N <= (1L << 60) / (C * H * W) && B <= (1L << 60) / (C * H * W),
              "%s: the store or the batch is too large to index (N, C, H, W, B = %ld, %ld, %ld, %ld, %ld)", name, N, C, H, W, B);
  const long esz = U8 ? 1 : 4, chw = C * H * W;
  AFD_REQUIRE(((uintptr_t)x & 3) == 0 && (U8 || ((uintptr_t)data & 3) == 0) && ((uintptr_t)idx & 7) == 0,
              "%s: x%s must be 4-byte aligned and idx 8-byte aligned", name, U8 ? "" : " and data");
  AFD_REQUIRE(!overlaps(x, B * chw * 4, data, N * chw * esz) && !overlaps(x, B * chw * 4, idx, B * 8) &&
                  !overlaps(x, B * chw * 4, flip, B) && !overlaps(x, B * chw * 4, table, C * 1024) &&
                  !overlaps(x, B * chw * 4, labels, N * 8) && !overlaps(x, B * chw * 4, y, B * 8),
              "%s: x must not overlap an input or y", name);
  const bool vec = (W * esz) % 16 == 0 && aligned16(data) && aligned16(x);      // then every plane and row starts 16-byte aligned
  const long plane = H * W;
  if (vec) {
    const long items = plane * esz / 16, by = (items + kVecThreads - 1) / kVecThreads;
    hipLaunchKernelGGL((batch_gather_k<U8, true, kVecThreads>), dim3((unsigned)(B * C), (unsigned)(by < kMaxPlaneBlocks ? by : kMaxPlaneBlocks)),
                       dim3(kVecThreads), 0, st, data, N, C, H, W, idx, flip, table, reinterpret_cast<uint32_t*>(x), labels, y);
  } else {
    const long by = (plane + kScalarThreads - 1) / kScalarThreads;
    hipLaunchKernelGGL((batch_gather_k<U8, false, kScalarThreads>), dim3((unsigned)(B * C), (unsigned)(by < kMaxPlaneBlocks ? by : kMaxPlaneBlocks)),
                       dim3(kScalarThreads), 0, st, data, N, C, H, W, idx, flip, table, reinterpret_cast<uint32_t*>(x), labels, y);
  }
  return check_launch(name);
}

extern "C" {

int afd_batch_gather_u8(const uint8_t* data, long N, long C, long H, long W, const int64_t* idx, const uint8_t* flip,
                        const float* table, float* x, const int64_t* labels, int64_t* y, long B, afd_stream_t st) {
  AFD_REQUIRE(data && idx && table && x, "afd_batch_gather_u8: data, idx, table and x must not be NULL");
  AFD_REQUIRE(((uintptr_t)table & 3) == 0, "afd_batch_gather_u8: table must be 4-byte aligned");
  return launch_batch_gather<true>("afd_batch_gather_u8", data, N, C, H, W, idx, flip, table, x, labels, y, B, as_stream(st));
}

int afd_batch_gather_f32(const float* data, long N, long C, long H, long W, const int64_t* idx, const uint8_t* flip, float* x,
                         const int64_t* labels, int64_t* y, long B, afd_stream_t st) {
  AFD_REQUIRE(data && idx && x, "afd_batch_gather_f32: data, idx and x must not be NULL");
  return launch_batch_gather<false>("afd_batch_gather_f32", data, N, C, H, W, idx, flip, nullptr, x, labels, y, B, as_stream(st));
}

}  // extern "C"

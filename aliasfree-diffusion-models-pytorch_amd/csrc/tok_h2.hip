// tok_h2.hip -- the token-wise chains of SelfAttention (see tok.hip) at C = 64 and C = 128 with every product on the fp16
// matrix pipe: two fp16 pieces per operand under power-of-two scales ("f16x2", h2_common.h), three cross terms (a1 b1,
// a2 b1, a1 b2) of v_mfma_f32_32x32x16_f16 per 16 channels of k.  A C = 128 product of one 32-token tile is 96 such
// instructions (3072 cycles) where the fp32 instruction needs 256 (16384 cycles), so ONE wave carries its tile through the
// whole chain in registers at every width, as the narrow fp32 kernels do at C = 32: no split of a tile over waves, no
// exchange tile, no redundant LayerNorm, every activation tensor read once (two deliberate exceptions, marked where they are).
//
// Operand layout.  The accumulator of 32x32x16_f16 is that of 32x32x2_f32 (T layout, tok_common.h): lane (pixel l31, half
// h), register r of block j = channel 32 j + (r & 3) + 8 (r >> 2) + 4 h.  Registers 8 s .. 8 s + 7 of a block, converted
// to fp16, are the 8 k-slots of lane half h in k-step (j, s): element e is channel 32 j + 16 s + 8 (e >> 2) + 4 h + (e & 3).
// The weight image holds its k in that same order: record (piece, G = 2 (2 j + s) + h, n) = the 8 fp16 of row n for those
// 8 channels; LDS [piece 2][G C/8][n C][8 fp16], so lane (n = l31, h) reads one 16-byte record per MFMA and the 32 lanes of
// a half read 512 contiguous bytes (conflict-free ds_read_b128).
//
// Scales.  Activations: one power of two PER TOKEN (LayerNorm re-normalises every token, so a token far below its tile's
// maximum must keep all its bits): the maximum over the lane's registers and one exchange with the partner lane
// (l31, 1 - h); undone in that lane's accumulator column.  Weights: one power of two per output row n (1 / s_n kept in LDS,
// applied with the bias).  Zeros give exact zeros, an inf / NaN stays inside its own token's column (h2_common.h rules).
//
// Weights.  The workgroup builds each image itself from the fp32 parameters (scalar loads: parameters sit at arbitrary
// 4-byte offsets), transposed for the backward forms, reading each matrix once (h2_stage below).  C = 64 keeps three
// images resident (48 KB); C = 128 (64 KB per image) runs the three products over TWO slots, the third matrix replacing the
// first behind the barriers of every pass, exactly as the fp32 chain kernels do.
#include "tok_common.h"
#include "h2_common.h"
#include "tok_h2.h"
#include <algorithm>

namespace afd {

// global <-> registers in T layout, written as (uniform row pointer)[per-lane offset]: the 32 C row offsets of a tile stay on
// the scalar side instead of one vector register each (the chains here hold three C-channel tiles at C = 128).
// Loads are unconditional: a lane past the last pixel reads pixel 0 of image 0 (pix_of clamps it), computes on it and
// stores nothing -- every quantity of a chain is private to its lane pair, and a select or a branch per element would
// cut the kernels into a hundred basic blocks that nothing can be scheduled across.
template <int NB>
__device__ __forceinline__ void h_load(TT<NB>& z, const float* __restrict__ src, unsigned base, int P) {
#pragma unroll
  for (int j = 0; j < NB; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) z.b[j][r] = (src + (size_t)tch(j, r) * P)[base];
}
template <int NB>
__device__ __forceinline__ void h_store(const TT<NB>& z, float* __restrict__ dst, unsigned base, int P, bool live) {
  if (!live) return;
#pragma unroll
  for (int j = 0; j < NB; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) (dst + (size_t)tch(j, r) * P)[base] = z.b[j][r];
}

template <int KB> struct HP { h8 a[2 * KB], b[2 * KB]; };        // the two pieces of a tile, one fragment per k-step

// split a tile under its per-token scale s; returns 1 / s
template <int KB>
__device__ __forceinline__ float hp_split(const TT<KB>& z, HP<KB>& p) {
  float m = 0.f;
#pragma unroll
  for (int j = 0; j < KB; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) m = fmaxf(m, fabsf(z.b[j][r]));
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  const float s = h2_scale_for(m);
#pragma unroll
  for (int k = 0; k < 2 * KB; ++k) {
    float x[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = z.b[k >> 1][8 * (k & 1) + e];
    h2_split8(x, s, p.a[k], p.b[k]);
  }
  return h2_inv_pow2(s);
}

// one 32-channel output block: s_tok s_n (W[nb*32 .. +32][:] . z) on the image `img`
template <int KB>
__device__ __forceinline__ f32x16 hp_block(const h8* __restrict__ img, int nb, int l31, int half, const HP<KB>& z) {
  constexpr int C = 32 * KB, NG = C / 8;
  const h8* __restrict__ w0 = img + half * C + nb * 32 + l31;
  const h8* __restrict__ w1 = w0 + NG * C;
  f32x16 acc = zero16();
#pragma unroll
  for (int k = 0; k < 2 * KB; ++k) {
    const h8 a1 = w0[2 * k * C], a2 = w1[2 * k * C];
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a2, z.a[k], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, z.b[k], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, z.a[k], acc, 0, 0, 0);
  }
  return acc;
}

// LDS of a workgroup: the image slots, per slot 1 / s_n and the row maxima of the build, then the kernel's vectors
template <int C> struct H2Lds {
  static constexpr int NG = C / 8, REC = 2 * NG * C;             // 16-byte records per image
  static constexpr bool RELOAD = C > 64;
  static constexpr int NSLOT = RELOAD ? 2 : 3;
  h8* img[3];
  float* winv[3];
  unsigned* rmax[3];
  float* vec;
  __device__ __forceinline__ void init(unsigned char* base) {
    h8* i0 = reinterpret_cast<h8*>(base);
    float* w0 = reinterpret_cast<float*>(i0 + NSLOT * REC);
    unsigned* r0 = reinterpret_cast<unsigned*>(w0 + NSLOT * C);
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      const int s = m % NSLOT;                                   // matrix 2 of a RELOAD chain lives in slot 0
      img[m] = i0 + s * REC; winv[m] = w0 + s * C; rmax[m] = r0 + s * C;
    }
    vec = reinterpret_cast<float*>(r0 + NSLOT * C);
  }
  static size_t bytes(int nvec) { return (size_t)NSLOT * REC * 16 + (size_t)NSLOT * C * 8 + (size_t)nvec * C * 4; }
};

// Building the images.  A matrix is named by its source: forward A[n][k] = w[(n0 + n) * ldw + k0 + k]; transposed (dgrad)
// A[n][k] = w[(k0 + k) * ldw + n0 + n].  The workgroup reads each matrix ONCE: a thread owns C * C / 8 / NT records, loads
// their 8 values each into registers (all loads of all matrices of a call in flight together: the build is one trip to
// L2, not one per row), folds their maxima into the rows' maxima in LDS (non-negative floats order as their bit patterns:
// one integer atomic max per record), and after a barrier splits its records under the row scales and stores them.
// Thread -> record: transposed, lanes along n (256-byte global runs, contiguous LDS stores); forward, 8 rows x 8 groups
// per wave (256-byte spans of 8 rows, LDS stores in contiguous 128-byte runs).
// All NT threads call h2_stage (it holds two barriers); the caller puts a barrier between the build and the first read
// of an image, and between the last read of a slot and its next build.
struct WSrc { const float* w; int ldw, n0, k0; };

template <int C, int NT> struct Stg {
  static constexpr int NG = C / 8, NR = C * NG / NT;
  float x[NR][8];
  static __device__ __forceinline__ void rec(int r, bool transposed, int& n, int& G) {
    const int i = (int)threadIdx.x + r * NT;
    if (transposed) { n = i % C; G = i / C; }
    else {
      const int lo = i & 63, hi = i >> 6;
      n = (hi % (C / 8)) * 8 + (lo & 7);
      G = (hi / (C / 8)) * 8 + (lo >> 3);
    }
  }
  __device__ __forceinline__ void load(const WSrc& q, bool transposed) {
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      int n, G;
      rec(r, transposed, n, G);
      const int kb = 16 * (G >> 1) + 4 * (G & 1);                 // 32 j + 16 s + 4 h
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int k = kb + 8 * (e >> 2) + (e & 3);
        x[r][e] = transposed ? q.w[(long)(q.k0 + k) * q.ldw + q.n0 + n] : q.w[(long)(q.n0 + n) * q.ldw + q.k0 + k];
      }
    }
  }
  __device__ __forceinline__ void maxima(unsigned* __restrict__ rmax, bool transposed) const {
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      int n, G;
      rec(r, transposed, n, G);
      float m = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) m = fmaxf(m, fabsf(x[r][e]));
      atomicMax(&rmax[n], __float_as_uint(m));
    }
  }
  __device__ __forceinline__ void store(h8* __restrict__ img, float* __restrict__ winv, const unsigned* __restrict__ rmax,
                                        bool transposed) const {
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      int n, G;
      rec(r, transposed, n, G);
      const float sc = h2_scale_for(__uint_as_float(rmax[n]));
      h8 p0, p1;
      h2_split8(x[r], sc, p0, p1);
      img[G * C + n] = p0;
      img[(NG + G) * C + n] = p1;
      if (G == 0) winv[n] = h2_inv_pow2(sc);
    }
  }
};

// build the images of matrices M0 .. M0 + CNT - 1 of the chain from src[0 .. CNT)
template <int C, int NT, int M0, int CNT>
__device__ __forceinline__ void h2_stage(const H2Lds<C>& L, const WSrc* src, bool transposed) {
  Stg<C, NT> st[CNT];
#pragma unroll
  for (int i = 0; i < CNT; ++i) st[i].load(src[i], transposed);
#pragma unroll
  for (int i = 0; i < CNT; ++i)
    for (int c = threadIdx.x; c < C; c += NT) L.rmax[M0 + i][c] = 0u;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < CNT; ++i) st[i].maxima(L.rmax[M0 + i], transposed);
  __syncthreads();
#pragma unroll
  for (int i = 0; i < CNT; ++i) st[i].store(L.img[M0 + i], L.winv[M0 + i], L.rmax[M0 + i], transposed);
  __builtin_amdgcn_sched_barrier(0);     // the build's value registers die here, before the next product's tiles are born
}
// the prologue (matrices 0, 1 and, where three slots exist, 2) and a single matrix
template <int C, int NT>
__device__ __forceinline__ void h2_stage_first(const H2Lds<C>& L, const WSrc* src, bool transposed) {
  if (H2Lds<C>::RELOAD) h2_stage<C, NT, 0, 2>(L, src, transposed);
  else h2_stage<C, NT, 0, 3>(L, src, transposed);
}
template <int C, int NT, int M>
__device__ __forceinline__ void h2_stage_one(const H2Lds<C>& L, const WSrc* src, bool transposed) {
  h2_stage<C, NT, M, 1>(L, src + M, transposed);
}

// the walk of a persistent workgroup of TPW waves over the pixel tiles
struct Walk { int lane, wv, half, l31, ntile, tstride, t0, npass; unsigned total; };
template <int TPW> __device__ __forceinline__ Walk walk_of(int B, int P) {
  Walk k;
  k.lane = threadIdx.x & 63; k.wv = threadIdx.x >> 6; k.half = k.lane >> 5; k.l31 = k.lane & 31;
  k.total = (unsigned)B * (unsigned)P;
  k.ntile = (int)((k.total + 31u) / 32u);
  k.tstride = gridDim.x * TPW;
  k.t0 = blockIdx.x * TPW;
  k.npass = k.t0 < k.ntile ? (k.ntile - k.t0 + k.tstride - 1) / k.tstride : 0;   // the same for every wave (barriers)
  return k;
}

extern __shared__ __attribute__((aligned(16))) unsigned char h2_smem[];

// ---------------------------------------------------------------------------------------------------------------------
// head forward: h = LN1(x); qkv = W_in h + b_in.  The three C-row slabs of W_in are the three matrices of the chain.
// ---------------------------------------------------------------------------------------------------------------------
template <int C, int TPW>
__global__ __launch_bounds__(64 * TPW) void tok_h2_head_fwd_k(const float* __restrict__ x, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, const float* __restrict__ w,
                                                               const float* __restrict__ bias, float* __restrict__ h_out,
                                                               float* __restrict__ stats_out, float* __restrict__ y, int B, int P,
                                                               float eps) {
  using LD = H2Lds<C>;
  constexpr int KB = C / 32, NT = 64 * TPW;
  LD L;
  L.init(h2_smem);
  float* vec = L.vec;                                             // gamma, beta, b_in[3C]
  const Walk k = walk_of<TPW>(B, P);
  const int half = k.half, l31 = k.l31;
  const WSrc src[3] = {{w, C, 0, 0}, {w, C, C, 0}, {w, C, 2 * C, 0}};
  h2_stage_first<C, NT>(L, src, false);
  for (int i = threadIdx.x; i < C; i += NT) { vec[i] = gamma[i]; vec[C + i] = beta[i]; }
  for (int i = threadIdx.x; i < 3 * C; i += NT) vec[2 * C + i] = bias ? bias[i] : 0.f;
  __syncthreads();
  for (int pass = 0; pass < k.npass; ++pass) {
    const int t = k.t0 + k.wv + pass * k.tstride;
    const bool active = t < k.ntile;                              // wave-uniform
    if (LD::RELOAD && pass > 0) { __syncthreads(); h2_stage_one<C, NT, 0>(L, src, false); __syncthreads(); }
    Pix pc = pix_of(active ? t : 0, l31, k.total, P);
    pc.live = pc.live && active;
    const unsigned yb = tbase(pc, 3 * C, P, half);
    HP<KB> hp;
    float is = 0.f;
    if (active) {
      const unsigned base = tbase(pc, C, P, half);
      TT<KB> xc, h;
      h_load(xc, x, base, P);
      float mean, rstd;
      t_ln_fwd<KB>(xc, vec, vec + C, half, eps, h, mean, rstd);
      if (h_out) h_store(h, h_out, base, P, pc.live);
      if (stats_out && pc.live && half == 0) { stats_out[2 * pc.f] = mean; stats_out[2 * pc.f + 1] = rstd; }
      is = hp_split<KB>(h, hp);
    }
#pragma unroll
    for (int sl = 0; sl < 3; ++sl) {
      if (LD::RELOAD && sl == 1) { __syncthreads(); h2_stage_one<C, NT, 2>(L, src, false); }
      if (LD::RELOAD && sl == 2) __syncthreads();
      if (active) {
#pragma unroll
        for (int nb = 0; nb < KB; ++nb) {
          const f32x16 acc = hp_block<KB>(L.img[sl], nb, l31, half, hp);
          if (pc.live) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int c = nb * 32 + tch(0, r) + 4 * half;
              (y + (size_t)(sl * C + nb * 32 + tch(0, r)) * P)[yb] = acc[r] * is * L.winv[sl][c] + vec[2 * C + sl * C + c];
            }
          }
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// tail forward: a = W_o att + b_o + x;  f = LN2(a);  u = W_1 f + b_1;  g = GELU(u);  out = W_2 g + b_2 + a.
// TRAIN also writes a, the LN2 statistics, f, u and g; the two forms differ in nothing else (bit-equal outputs).
// ---------------------------------------------------------------------------------------------------------------------
template <int C, int TPW, bool TRAIN>
__global__ __launch_bounds__(64 * TPW) void tok_h2_tail_fwd_k(const float* __restrict__ att, const float* __restrict__ xres,
                                                               const float* __restrict__ wo, const float* __restrict__ bo,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta,
                                                               const float* __restrict__ w1, const float* __restrict__ b1,
                                                               const float* __restrict__ w2, const float* __restrict__ b2,
                                                               float* __restrict__ a_out, float* __restrict__ stats_out,
                                                               float* __restrict__ f_out, float* __restrict__ u_out,
                                                               float* __restrict__ g_out, float* __restrict__ out, int B, int P,
                                                               float eps) {
  using LD = H2Lds<C>;
  constexpr int KB = C / 32, NT = 64 * TPW;
  LD L;
  L.init(h2_smem);
  float* vec = L.vec;                                             // bo, gamma, beta, b1, b2
  const Walk k = walk_of<TPW>(B, P);
  const int half = k.half, l31 = k.l31;
  const WSrc src[3] = {{wo, C, 0, 0}, {w1, C, 0, 0}, {w2, C, 0, 0}};
  h2_stage_first<C, NT>(L, src, false);
  for (int i = threadIdx.x; i < C; i += NT) {
    vec[i] = bo[i]; vec[C + i] = gamma[i]; vec[2 * C + i] = beta[i]; vec[3 * C + i] = b1[i]; vec[4 * C + i] = b2[i];
  }
  __syncthreads();
  for (int pass = 0; pass < k.npass; ++pass) {
    const int t = k.t0 + k.wv + pass * k.tstride;
    const bool active = t < k.ntile;
    if (LD::RELOAD && pass > 0) { __syncthreads(); h2_stage_one<C, NT, 0>(L, src, false); __syncthreads(); }
    Pix pc = pix_of(active ? t : 0, l31, k.total, P);
    pc.live = pc.live && active;
    const unsigned base = tbase(pc, C, P, half);
    TT<KB> a;
    HP<KB> hp;
    float is = 0.f;
    if (active) {
      TT<KB> z, xr;
      h_load(z, att, base, P);
      h_load(xr, xres, base, P);
      is = hp_split<KB>(z, hp);
#pragma unroll
      for (int nb = 0; nb < KB; ++nb) {
        const f32x16 acc = hp_block<KB>(L.img[0], nb, l31, half, hp);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int c = nb * 32 + tch(0, r) + 4 * half;
          a.b[nb][r] = acc[r] * is * L.winv[0][c] + vec[c] + xr.b[nb][r];
        }
      }
      float mean, rstd;
      t_ln_fwd<KB>(a, vec + C, vec + 2 * C, half, eps, z, mean, rstd);          // z = f
      if (TRAIN) {
        h_store(a, a_out, base, P, pc.live);
        h_store(z, f_out, base, P, pc.live);
        if (pc.live && half == 0) { stats_out[2 * pc.f] = mean; stats_out[2 * pc.f + 1] = rstd; }
      }
      is = hp_split<KB>(z, hp);
    }
    if (LD::RELOAD) { __syncthreads(); h2_stage_one<C, NT, 2>(L, src, false); }
    if (active) {
      TT<KB> g;
#pragma unroll
      for (int nb = 0; nb < KB; ++nb) {
        const f32x16 acc = hp_block<KB>(L.img[1], nb, l31, half, hp);
        TT<1> ub;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int c = nb * 32 + tch(0, r) + 4 * half;
          ub.b[0][r] = acc[r] * is * L.winv[1][c] + vec[3 * C + c];
          g.b[nb][r] = gelu_erf(ub.b[0][r]);
        }
        if (TRAIN) h_store(ub, u_out + (size_t)(32 * nb) * P, base, P, pc.live);
      }
      if (TRAIN) h_store(g, g_out, base, P, pc.live);
      is = hp_split<KB>(g, hp);
    }
    if (LD::RELOAD) __syncthreads();
    if (active) {
#pragma unroll
      for (int nb = 0; nb < KB; ++nb) {
        // TRAIN at C = 128 reads a back, block by block, from a_out (this lane's own stores of a moment ago: L2): through
        // the last two products a would be a third tile beside the operand pieces and g, with the stores of f, u and g
        // in flight.  The same bits either way, so the two forms stay bit-equal.
        TT<1> ar;
        if (TRAIN && KB > 2) h_load(ar, a_out + (size_t)(32 * nb) * P, base, P);
        else ar.b[0] = a.b[nb];
        const f32x16 acc = hp_block<KB>(L.img[2], nb, l31, half, hp);
        if (pc.live) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int c = nb * 32 + tch(0, r) + 4 * half;
            (out + (size_t)tch(nb, r) * P)[base] = acc[r] * is * L.winv[2][c] + vec[4 * C + c] + ar.b[0][r];
          }
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// tail backward: du = (W2^T d_out) * GELU'(u);  df = W1^T du;  d_a = LN2'(df; a) + d_out;  d_att = Wo^T d_a
// ---------------------------------------------------------------------------------------------------------------------
template <int C, int TPW>
__global__ __launch_bounds__(64 * TPW) void tok_h2_tail_bwd_k(const float* __restrict__ dout, const float* __restrict__ u_in,
                                                               const float* __restrict__ a_in, const float* __restrict__ stats,
                                                               const float* __restrict__ gamma, const float* __restrict__ w2,
                                                               const float* __restrict__ w1, const float* __restrict__ wo,
                                                               float* __restrict__ du_out, float* __restrict__ df_out,
                                                               float* __restrict__ da_out, float* __restrict__ datt_out, int B,
                                                               int P) {
  using LD = H2Lds<C>;
  constexpr int KB = C / 32, NT = 64 * TPW;
  LD L;
  L.init(h2_smem);
  float* gs = L.vec;
  const Walk k = walk_of<TPW>(B, P);
  const int half = k.half, l31 = k.l31;
  const WSrc src[3] = {{w2, C, 0, 0}, {w1, C, 0, 0}, {wo, C, 0, 0}};
  h2_stage_first<C, NT>(L, src, true);
  for (int i = threadIdx.x; i < C; i += NT) gs[i] = gamma[i];
  __syncthreads();
  for (int pass = 0; pass < k.npass; ++pass) {
    const int t = k.t0 + k.wv + pass * k.tstride;
    const bool active = t < k.ntile;
    if (LD::RELOAD && pass > 0) { __syncthreads(); h2_stage_one<C, NT, 0>(L, src, true); __syncthreads(); }
    Pix pc = pix_of(active ? t : 0, l31, k.total, P);
    pc.live = pc.live && active;
    const unsigned base = tbase(pc, C, P, half);
    HP<KB> hp;
    float is = 0.f;
    if (active) {
      TT<KB> z, uu;
      h_load(z, dout, base, P);
      h_load(uu, u_in, base, P);
      is = hp_split<KB>(z, hp);
#pragma unroll
      for (int nb = 0; nb < KB; ++nb) {
        const f32x16 acc = hp_block<KB>(L.img[0], nb, l31, half, hp);
#pragma unroll
        for (int r = 0; r < 16; ++r)
          z.b[nb][r] = acc[r] * is * L.winv[0][nb * 32 + tch(0, r) + 4 * half] * gelu_erf_grad(uu.b[nb][r]);
      }
      h_store(z, du_out, base, P, pc.live);                                       // du
      is = hp_split<KB>(z, hp);
    }
    if (LD::RELOAD) { __syncthreads(); h2_stage_one<C, NT, 2>(L, src, true); }
    if (active) {
      TT<KB> df, aa, dd;
#pragma unroll
      for (int nb = 0; nb < KB; ++nb) {
        const f32x16 acc = hp_block<KB>(L.img[1], nb, l31, half, hp);
#pragma unroll
        for (int r = 0; r < 16; ++r) df.b[nb][r] = acc[r] * is * L.winv[1][nb * 32 + tch(0, r) + 4 * half];
      }
      h_store(df, df_out, base, P, pc.live);
      // d_out a second time (the residual branch), on purpose: held in registers through the first two products it would
      // be a fourth C-channel tile beside the operand pieces, df and a (256 + registers at C = 128: one wave per SIMD);
      // the lines are this wave's own of a moment ago, so the re-read is served by L2.
      h_load(dd, dout, base, P);
      h_load(aa, a_in, base, P);
      const float mean = pc.live ? stats[2 * pc.f] : 0.f, rstd = pc.live ? stats[2 * pc.f + 1] : 0.f;
      t_ln_bwd<KB>(df, aa, gs, half, mean, rstd, dd);                             // df := d_a
      h_store(df, da_out, base, P, pc.live);
      is = hp_split<KB>(df, hp);
    }
    if (LD::RELOAD) __syncthreads();
    if (active) {
#pragma unroll
      for (int nb = 0; nb < KB; ++nb) {
        const f32x16 acc = hp_block<KB>(L.img[2], nb, l31, half, hp);
        if (pc.live) {
#pragma unroll
          for (int r = 0; r < 16; ++r)
            (datt_out + (size_t)tch(nb, r) * P)[base] = acc[r] * is * L.winv[2][nb * 32 + tch(0, r) + 4 * half];
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// head backward: dh = W_in^T dqkv (slab s of W_in: rows [sC, (s+1)C), A[n][k] = w_in[(sC + k) * C + n]);
// dx = LN1'(dh; x) + d_res.  Each slab of dqkv has its own per-token scale, so the three partial products meet in fp32.
// ---------------------------------------------------------------------------------------------------------------------
template <int C, int TPW>
__global__ __launch_bounds__(64 * TPW) void tok_h2_head_bwd_k(const float* __restrict__ dqkv, const float* __restrict__ x,
                                                               const float* __restrict__ stats, const float* __restrict__ gamma,
                                                               const float* __restrict__ w_in, const float* __restrict__ dres,
                                                               float* __restrict__ dh_out, float* __restrict__ dx_out, int B,
                                                               int P) {
  using LD = H2Lds<C>;
  constexpr int KB = C / 32, NT = 64 * TPW;
  LD L;
  L.init(h2_smem);
  float* gs = L.vec;
  const Walk k = walk_of<TPW>(B, P);
  const int half = k.half, l31 = k.l31;
  const WSrc src[3] = {{w_in, C, 0, 0}, {w_in, C, 0, C}, {w_in, C, 0, 2 * C}};
  h2_stage_first<C, NT>(L, src, true);
  for (int i = threadIdx.x; i < C; i += NT) gs[i] = gamma[i];
  __syncthreads();
  for (int pass = 0; pass < k.npass; ++pass) {
    const int t = k.t0 + k.wv + pass * k.tstride;
    const bool active = t < k.ntile;
    if (LD::RELOAD && pass > 0) { __syncthreads(); h2_stage_one<C, NT, 0>(L, src, true); __syncthreads(); }
    Pix pc = pix_of(active ? t : 0, l31, k.total, P);
    pc.live = pc.live && active;
    const unsigned base = tbase(pc, C, P, half);
    const unsigned qb = tbase(pc, 3 * C, P, half);
    TT<KB> dh;
#pragma unroll
    for (int sl = 0; sl < 3; ++sl) {
      if (LD::RELOAD && sl == 1) { __syncthreads(); h2_stage_one<C, NT, 2>(L, src, true); }
      if (LD::RELOAD && sl == 2) __syncthreads();
      if (active) {
        TT<KB> z;
        HP<KB> hp;
        h_load(z, dqkv + (size_t)(sl * C) * P, qb, P);
        const float is = hp_split<KB>(z, hp);
#pragma unroll
        for (int nb = 0; nb < KB; ++nb) {
          const f32x16 acc = hp_block<KB>(L.img[sl], nb, l31, half, hp);
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float v = acc[r] * is * L.winv[sl][nb * 32 + tch(0, r) + 4 * half];
            dh.b[nb][r] = sl == 0 ? v : dh.b[nb][r] + v;
          }
        }
      }
    }
    if (active) {
      if (dh_out) h_store(dh, dh_out, base, P, pc.live);
      TT<KB> xx, rr;
      h_load(xx, x, base, P);
      h_load(rr, dres, base, P);
      const float mean = pc.live ? stats[2 * pc.f] : 0.f, rstd = pc.live ? stats[2 * pc.f + 1] : 0.f;
      t_ln_bwd<KB>(dh, xx, gs, half, mean, rstd, rr);
      h_store(dh, dx_out, base, P, pc.live);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
// Waves (= tiles) per workgroup: four measured faster than two at C = 64 on both maps of the train step (B = 256, 16x16:
// 93 against 111 us over the four kernels; 8x8: 52 against 55), and the build of a C = 128 image wants the 256 threads.
// Workgroups beyond what the chip holds at once (C = 128: one per CU by LDS; C = 64: three) would only build the images
// again, so the grid is capped there and the workgroups walk.
static int g_h2_tpw = 0;              // tuning hook (afd_debug_tok_path 5 / 6): 2 or 4 waves per workgroup at C = 64, 0 = by the rule
void tok_h2_debug_tpw(int tpw) { g_h2_tpw = tpw; }
static int h2_tpw(long ntile) { (void)ntile; return g_h2_tpw ? g_h2_tpw : 4; }
static unsigned h2_grid(int C, long ntile, int tpw, int max_wg) {
  const long wg = (ntile + tpw - 1) / tpw;
  const long cap = max_wg > 0 ? max_wg : (C > 64 ? 256 : 768);
  return (unsigned)std::min<long>(wg, cap);
}

#define AFD_H2_LAUNCH(KERN, NVEC, ...)                                                                              \
  do {                                                                                                              \
    const size_t lds = H2Lds<KC>::bytes(NVEC);                                                                      \
    if (int rc = lds_opt_in(KERN, lds)) return rc;                                                                  \
    hipLaunchKernelGGL(KERN, dim3(h2_grid(KC, ntile, KT, max_wg)), dim3(64 * KT), lds, s, __VA_ARGS__);             \
  } while (0)
// runs BODY with KC / KT the compile-time C and waves per workgroup
#define AFD_H2_SWITCH(BODY)                                                                                         \
  do {                                                                                                              \
    if (C == 64) { constexpr int KC = 64; if (tpw == 4) { constexpr int KT = 4; BODY; } else { constexpr int KT = 2; BODY; } } \
    else         { constexpr int KC = 128; constexpr int KT = 4; BODY; }                                             \
  } while (0)

int tok_h2_head_fwd(const float* x, const float* gamma, const float* beta, const float* w, const float* bias, float* h_out,
                    float* stats_out, float* qkv, int B, int C, int P, float eps, int max_wg, hipStream_t s) {
  const long ntile = ((long)B * P + 31) / 32;
  const int tpw = h2_tpw(ntile);
  AFD_H2_SWITCH(AFD_H2_LAUNCH((tok_h2_head_fwd_k<KC, KT>), 5, x, gamma, beta, w, bias, h_out, stats_out, qkv, B, P, eps));
  return check_launch("afd_tok_head_fwd");
}

int tok_h2_tail_fwd(const float* att, const float* x, const float* wo, const float* bo, const float* gamma, const float* beta,
                    const float* w1, const float* b1, const float* w2, const float* b2, float* a_out, float* stats_out,
                    float* f_out, float* u_out, float* g_out, float* out, int B, int C, int P, float eps, int max_wg, hipStream_t s) {
  const long ntile = ((long)B * P + 31) / 32;
  const int tpw = h2_tpw(ntile);
  if (a_out)
    AFD_H2_SWITCH(AFD_H2_LAUNCH((tok_h2_tail_fwd_k<KC, KT, true>), 5, att, x, wo, bo, gamma, beta, w1, b1, w2, b2, a_out, stats_out,
                                f_out, u_out, g_out, out, B, P, eps));
  else
    AFD_H2_SWITCH(AFD_H2_LAUNCH((tok_h2_tail_fwd_k<KC, KT, false>), 5, att, x, wo, bo, gamma, beta, w1, b1, w2, b2, a_out, stats_out,
                                f_out, u_out, g_out, out, B, P, eps));
  return check_launch("afd_tok_tail_fwd");
}

int tok_h2_tail_bwd(const float* d_out, const float* u, const float* a, const float* stats, const float* gamma, const float* w2,
                    const float* w1, const float* wo, float* du_out, float* df_out, float* da_out, float* datt_out, int B, int C,
                    int P, int max_wg, hipStream_t s) {
  const long ntile = ((long)B * P + 31) / 32;
  const int tpw = h2_tpw(ntile);
  AFD_H2_SWITCH(AFD_H2_LAUNCH((tok_h2_tail_bwd_k<KC, KT>), 1, d_out, u, a, stats, gamma, w2, w1, wo, du_out, df_out, da_out, datt_out,
                              B, P));
  return check_launch("afd_tok_tail_bwd");
}

int tok_h2_head_bwd(const float* dqkv, const float* x, const float* stats, const float* gamma, const float* w_in,
                    const float* d_res, float* dh_out, float* dx_out, int B, int C, int P, int max_wg, hipStream_t s) {
  const long ntile = ((long)B * P + 31) / 32;
  const int tpw = h2_tpw(ntile);
  AFD_H2_SWITCH(AFD_H2_LAUNCH((tok_h2_head_bwd_k<KC, KT>), 1, dqkv, x, stats, gamma, w_in, d_res, dh_out, dx_out, B, P));
  return check_launch("afd_tok_head_bwd");
}

#undef AFD_H2_SWITCH
#undef AFD_H2_LAUNCH

}  // namespace afd

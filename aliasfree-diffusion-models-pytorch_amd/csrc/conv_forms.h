// conv_forms.h -- the convolution family's cross-file surface (internal): the switches behind afd_debug_conv_path, and every host
// function that one of conv / pw / ends / wino / bf3 / h2 / bf3_wgrad / h2_wgrad / fold.hip defines and another calls.  All of them
// include it, the defining file too: a definition that drifts from its declaration no longer compiles.  New launchers go here.
#pragma once
#include "common.h"

namespace afd {

// One member per value afd_debug_conv_path can set (conv.hip: kConvModes maps mode numbers to members), all long;
// afd_debug_conv_state reads them back in this order.  A new switch = a member here, its rows in kConvModes, a line in afd.h.
struct ConvSwitches {
  long tile_path = 0;       // 0 auto, 1 force the 64x128 tile, 2 force the split-K small tile (tests)
  long pw_mode = 0;         // 1x1 streaming kernel (pw.hip): 0 = by the measured rule, 1 = never, 2 = whenever the shape is covered
  long wgrad_nw = 0;        // tuning hook: waves per fp32 wgrad workgroup (0 = chosen per layer)
  long wgb_target = 256;    // matrix-core 3x3 wgrad, workgroups per launch: 256 standalone, 160 beside the chain (48 / 49)
  long wg_waves_mode = 0;   // 50 ... 55: waves per workgroup of the f16x2 3x3 wgrad (bf3_wgrad.hip: wgrad_four_waves)
  long h2_lds = 1;          // 60 (by rule, default) / 61 (the register-fed kernel) / 62, 63, 59 (tests: LDS-fed wherever covered, (128, 2) / (256, 1) / (128, 1) first) = 1 / 0 / 2, 3, 4
  long wino_mode = 0;       // 0 = by rule, 1 = off, 2..5 = whenever the shape is supported: workgroups of 64x64, 32x64, 64x32, 32x32 (channels x tiles); 6 = the small-map split-K kernel wherever covered
  long h2_skw = 0;          // 71 / 72: the slice-walking split-K kernel wherever SW >= 2 is possible (tests) / never; 74 = by rule (default)
  long sk_mode = 0;         // 74 / 75 / 73: the f16x2 split-K kernel by the rule / never / wherever the shape is covered (ahead of the tile kernel)
  long direct_bf3 = 0;      // 76 / 77: the direct form is f16x2 (h2.hip, default) / bf16x3 (bf3.hip)
  long wg_arith_bf3 = 0;    // 78 / 79: the 3x3 weight gradient's arithmetic is f16x2 (h2_wgrad.hip, default) / bf16x3 (bf3_wgrad.hip)
  long bf3_mode = 0;        // 80 / 81 / 82: the direct matrix-core form by the rule / off / wherever the shape is covered
  long wgbf3_mode = 0;      // 84 / 85 / 86: the matrix-core wgrad by the rule / off / wherever the shape is covered
  long pwbf3_mode = 0;      // 88 / 89: the 1x1 matrix-core wgrad by the rule / off
  long ends_mode = 0;       // 92 / 93: the output-layer kernels (ends.hip) by the rule / never
  long wgwino_mode = 0;     // 96 / 97 / 98: the Winograd wgrad by rule / off / whenever covered
  long wino_grid = 0;       // 100000 + g, test / tuning hook: persistent Winograd grid size (0 = one item per workgroup)
};
constexpr int kConvSwitchCount = sizeof(ConvSwitches) / sizeof(long);
extern ConvSwitches g_conv;                                             // conv.hip

// ---- pw.hip, ends.hip: true = the kernel took the layer and was launched, false = the caller goes on to the next form
bool pw_launch(const float* in, const float* w, const float* bias, const float* res, float* out, int B, int K, int N, int P,
               int act, bool dgrad, hipStream_t s);
bool ends_fwd(const float* x, const float* w, const float* bias, const float* res, float* y, int B, int Cin, int Cout, int H, int W,
              int ksize, int act, hipStream_t s);
bool ends_dgrad(const float* dy, const float* w, float* dx, int B, int Cin, int Cout, int H, int W, int ksize, hipStream_t s);

// ---- wino.hip: wino_plan = workgroup shape BN * 256 + NT (1 = the small-map kernel, 0 = not covered); wgrad_wino_plan = slabs
// (0 = not covered); wino_conv = -1 not covered, else AFD_OK or a launcher's code; wgrad_wino = slabs > 0 launched, 0 not
// covered, -code on a failed LDS opt-in (nothing launched)
int wino_plan(int B, int K, int N, int H, int W);
int wgrad_wino_plan(int B, int Cin, int Cout, int H, int W, int* bn, int* bk, int* cps, int* nchunks);
int wino_conv(const float* x, const float* w, const float* bias, const float* res, float* y, float* U, int B, int K, int N, int H,
              int W, int act, bool dgrad, bool weights_ready, hipStream_t s);
int wgrad_wino(const float* x, const float* dy, float* part, int B, int Cin, int Cout, int H, int W, hipStream_t s);
void wino_weights_launch(const float* w, float* Uf, float* Ud, int Cin, int Cout, int kinds, hipStream_t s);
void wino_weights_batched_launch(const afd_wino_desc* descs, const int* wg_desc, int n_wg, hipStream_t s);

// ---- bf3.hip: direct_plan = 0 no direct form, 1 the 128-pixel tile kernel, 2 the split-K small-map kernel; bf3_ok = plan != 0
int direct_plan(int B, int K, int N, int H, int W);
bool bf3_ok(int B, int K, int N, int H, int W);
void bf3_weights_launch(const float* w, void* Wf, void* Wd, int Cin, int Cout, hipStream_t s);
void bf3_conv(const float* x, const void* Wp, const float* bias, const float* res, float* y, int B, int K, int N, int S, int act, hipStream_t s);

// ---- h2.hip: h2_sk_ok = the split-K small-map kernel covers the shape; h2_conv = AFD_OK or a failed LDS opt-in's code (nothing launched)
bool h2_sk_ok(int B, int K, int N, int H, int W, bool force);
void h2_weights_launch(const float* w, void* Wf, void* Wd, int Cin, int Cout, hipStream_t s);
int h2_conv(const float* x, const void* Wp, const float* bias, const float* res, float* y, int B, int K, int N, int S, int act,
            hipStream_t s, bool small);

// ---- bf3_wgrad.hip, h2_wgrad.hip: all return the slabs, 0 = not covered or switched off; launchers: -code on a failed LDS opt-in (nothing launched)
int wgrad_plan_full(int B, int Cin, int Cout, int H, int W, int* tps, int* ntiles, int* bn, int* bk, int* nw);
int wgrad_bf3_plan(int B, int Cin, int Cout, int H, int W, int* tps, int* ntiles);
int pw_wgrad_bf3_plan(int B, int Cin, int Cout, int L, int* sps, int* nsteps, int* nr, int* nt);
int wgrad_cin3_plan(int B, int Cin, int Cout, int H, int W);
int wgrad_bf3(const float* x, const float* dy, float* part, int B, int Cin, int Cout, int H, int W, hipStream_t s);
int pw_wgrad_bf3(const float* x, const float* dy, float* part, float* bias_part, int B, int Cin, int Cout, int L, hipStream_t s);
int wgrad_cin3(const float* x, const float* dy, float* part, int B, int Cin, int Cout, int H, int W, hipStream_t s);
int wgrad_h2(const float* x, const float* dy, float* part, int B, int Cin, int Cout, int H, int W, hipStream_t s);
int pw_wgrad_h2(const float* x, const float* dy, float* part, float* bias_part, int B, int Cin, int Cout, int L, hipStream_t s);

// ---- fold.hip: AFD_OK, or AFD_EINVAL for a bad descriptor (nothing launched from that batch on)
int fold_launch(const afd_fold_desc* descs, int n, hipStream_t s);

}  // namespace afd

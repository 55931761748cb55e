// The "thin" conv1d path (conv1d_thin.hip): kernels for single-input-channel layers with short kernels - Cin = 1,
// k = 25, stride 4, the first conv of the audio critic and of WaveGAN. With a contraction of 25 taps the layer is
// HBM-bound and the GEMM engine's 128-wide tiles would be mostly padding, so all three directions run on 32 x 32 MFMA
// tiles with the 32 channels as one tile dimension. conv1d.hip routes to these launchers where the *_applicable tests
// say so; everything else takes the engine.
#pragma once
#include "m2d_common.h"

// Window view of a padded track (B, S): the logical input is (B*T, 1, window), window t of track b
// starting at b*S + t*hop (utils.slice_audio_batch of the reference, never materialised). T == 0: dense.
struct M2dWinView {
  int T, S, hop;
};

bool m2d_thin_applicable(int Cin, int Cout, int ks, int stride);
bool m2d_thin_long_applicable(int Cin, int Cout, int ks, int stride, int pad, int L);
size_t m2d_thin_long_stats_ws(int B, int Lout);
int m2d_thin_long_fwd(const float* x, const float* w, const float* bias, float* y, int B, int L, int ks, int stride, int pad,
                      int Lout, int act, float slope, const M2dWinView* wv, double* stats, void* ws, size_t ws_bytes,
                      hipStream_t stream);
size_t m2d_thin_bwd_weight_ws(int B, int Cout, int ks, int Lout);
size_t m2d_thin_fwd_stats_ws(int B, int Lout);
int m2d_thin_fwd(const float* x, const float* w, const float* bias, float* y, int B, int L, int Cout, int ks,
                 int stride, int pad, int Lout, int act, float slope, const float* out_mask, float out_mask_slope,
                 const M2dWinView* wv, double* stats, void* ws, size_t ws_bytes, hipStream_t stream);
int m2d_thin_bwd_data(const float* dy, const float* w, float* dx, int B, int L, int Cout, int ks, int stride,
                      int pad, int Lout, const float* dy_mask, float dy_mask_slope, hipStream_t stream);
int m2d_thin_bwd_weight(const float* x, const float* dy, float* dw, float* dbias, int B, int L, int Cout, int ks,
                        int stride, int pad, int Lout, const float* dy_mask, float dy_mask_slope, void* ws,
                        size_t ws_bytes, const M2dWinView* wv, hipStream_t stream);

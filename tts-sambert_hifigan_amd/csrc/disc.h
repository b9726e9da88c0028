// disc.h — what the discriminators' units share: the kernel parameters and launchers
// (disc_conv.hip, disc_thin.hip), the weight packer (pack.cpp) and the C ABI (disc_capi.cpp,
// include/hifigan_hip_disc.h).  Every tensor is [B][C][H][W] float32 and every conv runs along
// H only: W is the period of a PeriodDiscriminator's fold and 1 for a ScaleDiscriminator.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "kernels.h"

namespace hfg {

// ---- disc_conv: grouped, strided implicit GEMM on the matrix cores (disc_conv.hip) ----
//   y[b][co][ho][w] = act(bias[co] + sum_{ci, t} Wt[co][ci][t] x[b][g cig + ci][ho s + t - pad][w])
// over the cig = C_in / groups channels of co's group g, x zero outside [0, H).
constexpr int kDiscNt = 64;       // output positions (ho, w) per block: 4 waves x 16 columns
constexpr int kDiscBandMax = 16;  // columns of W a block spans (wider W: bands of 16)
struct DiscConvParams {
  const float* x;      // [B][C_in][H][W]
  float* y;            // [B][C_out][H_out][W]
  const __bf16* w;     // packed f16 halves scaled by 2^ew (disc_conv_nest, pack_layout.h)
  const float* bias;   // [C_out]
  int C_in, C_out, groups;
  int H, W, H_out;
  int k, stride, pad;
  int act;             // leaky_relu(0.1) on the output
  int ew;              // the weights' packing exponent
};
// rows per block: 16 MSUB; the instance a group of cog output channels runs on
inline int disc_conv_msub(int cog) { return cog % 64 == 0 ? 4 : (cog % 32 == 0 ? 2 : 1); }
// columns per band, bands, and staged input rows of a block (the LDS formula's inputs)
inline int disc_conv_tw(int W) { return W < kDiscBandMax ? W : kDiscBandMax; }
int disc_conv_rows(int W, int k, int stride);
size_t disc_conv_lds_bytes(int cig, int W, int k, int stride);
bool disc_conv_supported(const DiscConvParams& p);
hipError_t launch_disc_conv(const DiscConvParams& p, int batch, hipStream_t stream,
                            const char** name);

// ---- thin ends, fp32 VALU (disc_thin.hip) ----
// entry conv, C_in = 1: the signal is src[b][0..T) read through the fold v[h][w] = src[h W + w]
// with the reference's right reflect pad fused (sample T + j reads T - 2 - j; the host has
// checked that it fits); y[b][co][ho][w] = lrelu(bias[co] + sum_t wt[co][t] v[ho s + t - pad][w])
struct DiscEntryParams {
  const float* src;    // [B][T]
  int64_t T;
  float* y;            // [B][C_out][H_out][W]
  const float* w;      // [C_out][k]
  const float* bias;   // [C_out]
  int C_out, H, W, H_out, k, stride, pad;
};
hipError_t launch_disc_entry(const DiscEntryParams& p, int batch, hipStream_t stream);
// conv_post, C_out = 1, k = 3, pad 1, no activation: y[b][h][w]; w: [C_in][3]
hipError_t launch_disc_post(const float* x, int C_in, int H, int W, const float* w,
                            const float* bias, float* y, int batch, hipStream_t stream);
// AvgPool1d(4, 2, padding 2), count_include_pad: y[b][i] = (x[2i-2] + .. + x[2i+1]) / 4 with x
// zero outside [0, L); L_out = L / 2 + 1
hipError_t launch_disc_pool(const float* x, int64_t L, float* y, int batch, hipStream_t stream);

// ---- feature matching sums (disc_thin.hip) ----
// sums[b][i] = sum |fake_i[b] - real_i[b]| over the n[i] elements of item b's map i (float64):
// kDiscFmBlocks block partials per (item, map) in ws, then one wave per pair.  No atomics and
// a fixed order: item b's sums do not depend on the batch around it.
constexpr int kDiscMaxMaps = 8;
constexpr int kDiscFmBlocks = 64;
struct DiscFmArgs {
  const float* real[kDiscMaxMaps];
  const float* fake[kDiscMaxMaps];
  int64_t n[kDiscMaxMaps];   // elements per item
  int n_maps;
};
inline size_t disc_fm_workspace_bytes(int64_t B, int n_maps) {
  return sizeof(double) * (size_t)B * n_maps * kDiscFmBlocks;
}
hipError_t launch_disc_fm_sums(const DiscFmArgs& a, int batch, double* ws, double* sums,
                               hipStream_t stream);

}  // namespace hfg

namespace hfg_host {
// one layer's folded weight [C_out][cig][k] -> the disc_conv packing: f16 hi and lo planes of
// w 2^ew, ew from the layer's largest |w| (x3_exp_host); returns ew
int pack_disc_conv(const float* w, int cig, int cog, int k, int groups, int msub, uint16_t* dst);
// the inverse: plane `plane` (0 hi, 1 lo) of every weight, scaled back by 2^-ew, as fp32
// [C_out][cig][k]
void unpack_disc_conv(const uint16_t* src, int cig, int cog, int k, int groups, int msub,
                      int plane, int ew, float* w);
}  // namespace hfg_host

// lds_layout.h — the dynamic-LDS carve-up of every kernel family, stated once.  A kernel takes
// its offsets and strides from its layout, its launcher (and the plan, where it consults the
// size) takes the total from the same value: a row or a pad added here moves both sides.
// Included at the end of kernels.h, after pack_layout.h (it needs the tile configurations
// declared there, and the global slabs whose LDS copies it places).
//
// A layout whose inputs are all template arguments is a plain struct of ints filled by a
// constexpr function, evaluated at compile time in the kernel.  A term with a runtime input
// (window columns of a generic-tap conv, n_conv, n_fft, C) is a __host__ __device__ constexpr
// function of its own that returns one number, in the unit (bf16, floats or bytes, as named)
// of the pointer the kernel indexes: the kernel calls it where it forms that pointer and the
// total is summed from the same functions.  (Returning those from one struct-valued call
// moved the device code of every kernel that tried it; DESIGN.md, "LDS layouts".)
#pragma once

#include "kernels.h"

namespace hfg {

// ---- LDS-staged float4 epilogue (epilogue.h), conv1d_mfma_f32 and conv1d_bf16x3 ----
// each wave stages 32 accumulator rows x 32*WN columns, row stride padded by 8 floats; the
// staging overlays the main loop's buffers from byte 0
constexpr int epi_stage_row(int WN) { return 32 * WN + 8; }                   // floats
constexpr int epi_stage_wave(int WN) { return 32 * epi_stage_row(WN); }       // floats
constexpr size_t epi_stage_bytes(int threads, int WN) {
  return sizeof(float) * (size_t)(threads / 64) * epi_stage_wave(WN);
}

// ---- conv1d_bf16x3 (conv_bf16x3.hip) ----
// [WD weight slabs][2 input windows x (hi, lo) planes]; the AREG tiles have no slab ring, one
// plane row per staging task, and the m-tile's bias copy past the windows and the staging.
constexpr int kBf16x3XRow = 16;  // bf16 per staged row: 16 channels (32 B)
struct ConvBf16x3Lds {
  int slab;      // bf16 per chunk slab: the global slab (pack_layout.h), copied whole
  int xw_max;    // widest window the instantiation stages (sizes its staging registers)
  int xq;        // staging tasks per thread: (row, 8-channel half) pairs of xw_max rows
  int xrows;     // AREG: rows of a plane, one per staging task (>= xw_max)
  int hps;       // AREG: bf16 per half plane (8 channels, 16-B rows), padded by 64 B so that a
                 // ds_write_b128 lane group covers the 32 write banks once
  int x_off;     // bf16 offset of the input windows (past the slab ring)
  int xplane;    // bf16 per input plane
  int xbuf;      // bf16 per window: hi + lo planes
  int main_bytes;  // slab ring + 2 windows
  int bias_off;  // AREG: byte offset of the bias copy (MT floats)
  int total_epi, total_plain;  // bytes with / without the LDS-staged epilogue (p.epi_lds)
  constexpr int total(bool epi) const { return epi ? total_epi : total_plain; }
};
// bf16 per input plane of xw window columns (the tiles with a slab ring), rounded to 16 B
__host__ __device__ constexpr int bf16x3_xplane(int xw) { return (xw * kBf16x3XRow + 7) & ~7; }
// kt_max: the instantiation's taps (16 for the runtime-tap instances); xw: window columns of
// this launch, NTILE + (kt - 1) * dil
constexpr ConvBf16x3Lds conv_bf16x3_lds(const Bf16x3Cfg& t, int kt_max, int xw) {
  ConvBf16x3Lds l{};
  const int nt = t.threads();
  l.slab = conv_bf16x3_pack(t).slab;
  l.xw_max = t.NTILE() + ((kt_max - 1) * kMaxDil < kBf16x3MaxHalo ? (kt_max - 1) * kMaxDil
                                                                   : kBf16x3MaxHalo);
  l.xq = (2 * l.xw_max + nt - 1) / nt;
  l.xrows = l.xq * nt / 2;
  l.hps = l.xrows * 8 + 32;
  l.x_off = t.AREG ? 0 : t.WD * l.slab;
  l.xplane = t.AREG ? 2 * l.hps : bf16x3_xplane(xw);
  l.xbuf = 2 * l.xplane;
  l.main_bytes = (int)sizeof(__bf16) * (l.x_off + 2 * l.xbuf);
  const int stage = (int)epi_stage_bytes(nt, t.WN);
  l.bias_off = ((l.main_bytes > stage ? l.main_bytes : stage) + 15) & ~15;
  l.total_plain = t.AREG ? l.bias_off + t.MT() * (int)sizeof(float) : l.main_bytes;
  l.total_epi = t.AREG ? l.total_plain : (l.main_bytes > stage ? l.main_bytes : stage);
  return l;
}
constexpr int bf16x3_xw(const Bf16x3Cfg& t, int kt, int dil) { return t.NTILE() + (kt - 1) * dil; }

// ---- ups_bf16x3 (ups_bf16x3.hip) ----
// [2 A slabs][2 input windows x (hi, lo) planes]; all bytes
struct UpsLds {
  int slab;    // one 16-channel group's global slab (pack_layout.h), copied whole
  int xr;      // staged frames: [m0 - 4, m0 + NTILE + 4), quad-aligned
  int xplane;  // one bf16 plane [frame][16 ch]
  int xbuf;    // hi + lo
  int x_off;   // input windows: past the 2-slab ring
  int total;
};
constexpr UpsLds ups_lds(const UpsCfg& t) {
  UpsLds l{};
  l.slab = ups_pack(t).slab;
  l.xr = t.NTILE() + 8;
  l.xplane = l.xr * 32;
  l.xbuf = 2 * l.xplane;
  l.x_off = 2 * l.slab;
  l.total = l.x_off + 2 * l.xbuf;
  return l;
}

// ---- resblock_bf16x3 / resblock2_bf16x3 (resblock_body.h) ----
// [C/16 groups x 2 half-groups x (hi, lo) planes of [row][8 bf16]][n_conv * C biases]
// [16 per-wave maxima (f16x3)][diagnostic build: the clock stamps]; the fused conv_post stages
// its rows over the planes
struct RbLds {
  int rows;      // operand rows: the window plus rb_marg spare rows a side
  int ps;        // bytes per plane
  int hps;       // half-group: hi, lo planes
  int gs;        // 16-channel group
  int bias_off;  // bytes: past the operand planes
  int bias_conv; // floats: one conv's biases; the per-wave maxima follow n_conv of them
  int amax_n;    // floats: the per-wave maxima; the clock stamps follow them
  int ts_bytes;  // the clock stamps of a -DHFG_RB_TIMING=1 build (diag.h), else 0
  int post_row;  // fused conv_post: row stride of its staging (floats): the two lane halves'
                 // rows, 4 apart, land 32 banks apart
  constexpr size_t total(int n_conv) const {
    return (size_t)bias_off + sizeof(float) * ((size_t)n_conv * bias_conv + amax_n) + ts_bytes;
  }
};
constexpr RbLds rb_lds(int C, int nwin) {
  RbLds l{};
  l.rows = nwin + 2 * rb_marg(C, nwin);
  l.ps = l.rows * 16;
  l.hps = 2 * l.ps;
  l.gs = 2 * l.hps;
  l.bias_off = C / 16 * l.gs;
  l.bias_conv = C;
  l.amax_n = 16;
  l.ts_bytes = HFG_RB_TIMING ? kRbTs.slots * (int)sizeof(uint64_t) : 0;
  l.post_row = nwin + 8;
  return l;
}

// ---- mrf_thin (mrf_thin.hip): C operand rows of the window plus kThinMarg columns a side ----
struct ThinLds {
  int rs;     // row stride (floats)
  int total;  // bytes
};
constexpr ThinLds thin_lds(int C, int nwin) {
  ThinLds l{};
  l.rs = nwin + 2 * kThinMarg;
  l.total = (int)sizeof(float) * C * l.rs;
  return l;
}

// ---- mrf_thin_mfma (mrf_thin_mfma.hip) ----
// [kThinMfmaBufs operand buffers x (hi, lo) planes of [row][C bf16]][4 per-wave maxima]; bytes
struct ThinMfmaLds {
  int rows;      // the window plus kThinMarg rows a side
  int rb;        // one operand row of one plane
  int ps;        // one plane
  int amax_off;  // per-wave maxima (f16x3): past the operand buffers
  int total;
};
constexpr ThinMfmaLds thin_mfma_lds(int C, int nwin) {
  ThinMfmaLds l{};
  l.rows = nwin + 2 * kThinMarg;
  l.rb = 2 * C;
  l.ps = l.rows * l.rb;
  l.amax_off = kThinMfmaBufs * 2 * l.ps;
  l.total = l.amax_off + 4 * (int)sizeof(float);
  return l;
}

// ---- conv1d_mfma_f32 (conv_kernels.hip): two pipeline stages of [weight slab][input rows];
// floats; the weight slab is the global one (conv_f32_slab, pack_layout.h).  The LDS-staged
// epilogue runs only where its staging fits under them. ----
__host__ __device__ constexpr int conv_f32_nx(int CK, int xw) {
  return CK * xw;       // staged input: CK rows of the window
}
// one pipeline stage, the input rows rounded up to 16 B
__host__ __device__ constexpr int conv_f32_stage(int wchunk, int nx) {
  return wchunk + ((nx + 3) & ~3);
}
constexpr size_t conv_f32_lds_total(int MT, int CK, int kt, int xw) {
  return sizeof(float) * 2 * (size_t)conv_f32_stage(conv_f32_slab(MT, CK, kt), conv_f32_nx(CK, xw));
}

// ---- conv_post_tanh (conv_kernels.hip): [C x 7 weights, rounded up to 16 B][kConvPostCB
// input rows of a 256-sample tile plus its 6 halo columns]; floats ----
constexpr int kConvPostTile = 256;  // (kConvPostTaps: pack_layout.h)
constexpr int kConvPostXw = kConvPostTile + kConvPostTaps - 1;  // staged columns per row
// the input rows: past the weights
__host__ __device__ constexpr int conv_post_x_off(int C) { return (C * kConvPostTaps + 3) & ~3; }
constexpr size_t conv_post_lds_bytes(int C) {
  return sizeof(float) *
         ((size_t)conv_post_x_off(C) + (size_t)(C < kConvPostCB ? C : kConvPostCB) * kConvPostXw);
}

// ---- stft_power_mfma / mel_log (mel_kernels.hip): the DFT-GEMM pair; floats ----
// stft_power_mfma: the reflect-padded samples of a block's kStftFrames frames, stored skewed:
// sample i at i + i / hop, so the 32 frames a half-wave reads at one k (frame * hop + k) fall in
// 32 different banks.  mel_log: kMelLogFrames power rows of n_bins.
constexpr int kStftFrames = 32, kMelLogFrames = 16;
__host__ __device__ constexpr int stft_span(int hop, int n_fft) {
  return (kStftFrames - 1) * hop + n_fft;
}
__host__ __device__ constexpr int stft_sig_idx(int i, int hop) { return i + i / hop; }
constexpr size_t stft_lds_bytes(int n_fft, int hop) {
  const size_t span = (size_t)(kStftFrames - 1) * hop + n_fft;  // stft_span, past int
  return sizeof(float) * (span + span / hop + 1);
}
constexpr size_t mel_log_lds_bytes(int n_bins) {
  return sizeof(float) * (size_t)kMelLogFrames * n_bins;
}
constexpr size_t kMelDftMaxLds = 64 * 1024;  // both launched without raising the LDS limit
// What hfg_mel_create admits to the pair.  stft_lds_bytes is the size; the second term is the
// bound handles were created under before (the tile as if skewed once per 32 samples): it
// refuses spans of 15888 to about 16350 floats that would fit, and stays so that no
// configuration changes sides (tests/test_mel_lds_host.py).
constexpr bool mel_dft_fits(int n_fft, int hop) {
  return stft_lds_bytes(n_fft, hop) <= kMelDftMaxLds &&
         ((size_t)(kStftFrames - 1) * hop + n_fft) * 4 * 33 / 32 <= kMelDftMaxLds &&
         mel_log_lds_bytes(n_fft / 2 + 1) <= kMelDftMaxLds;
}

// ---- logmel_fft / release_mel_fft (mel_kernels.hip, mel_fft_body.h) ----
// [4 waves x 2 FFT buffers of n_fft/2 complex doubles][the block's sample span, fp32, rounded
// up to 16 B][n_mels x frames-per-block output tile, fp32]
__host__ __device__ constexpr int mel_fft_fpb(int fpw) { return 4 * fpw; }  // frames per block
// samples the block's frames cover
__host__ __device__ constexpr int mel_fft_span(int fpb, int hop, int n_fft) {
  return (fpb - 1) * hop + n_fft;
}
// bytes: the span, past the FFT buffers (n2 = n_fft / 2 complex doubles each)
__host__ __device__ constexpr size_t mel_fft_sig_off(int n2) { return 2 * sizeof(double) * 8 * n2; }
// floats past the span's start: the output tile
__host__ __device__ constexpr int mel_fft_mel_idx(int span) { return (span + 3) & ~3; }
constexpr size_t mel_fft_lds_total(int n_fft, int hop, int fpw, int n_mels) {
  const int fpb = mel_fft_fpb(fpw);
  return mel_fft_sig_off(n_fft / 2) +
         sizeof(float) * ((size_t)mel_fft_mel_idx(mel_fft_span(fpb, hop, n_fft)) +
                          (size_t)n_mels * fpb);
}

// ---- mel_distance_fft / stft_distance_fft (spectral_distance.hip) ----
// mel_distance_fft: the logmel_fft / release_mel_fft carve-up above (mel_fft_lds_total); the
// four waves' partial sums overlay the FFT buffers once the frames are done.
// stft_distance_fft: [the same FFT buffers][the block's span of signal a][of signal b], each
// span fp32 and rounded up to 16 B; the wave partials overlay the FFT buffers likewise.
__host__ __device__ constexpr int stft_dist_sig_stride(int span) { return (span + 3) & ~3; }  // floats
constexpr size_t stft_dist_lds_total(int n_fft, int hop, int fpw) {
  return mel_fft_sig_off(n_fft / 2) +
         sizeof(float) * 2 *
             (size_t)stft_dist_sig_stride(mel_fft_span(mel_fft_fpb(fpw), hop, n_fft));
}

// ---- resample_sinc / resample_ragged (resample.hip): [C channels][the input span of a
// block's 256 outputs], C = 1 for resample_sinc; floats.  The 256 outputs cover at most
// 255 / n_phases + 1 steps of `stride` input samples beyond the first output's klen taps. ----
__host__ __device__ constexpr int resample_span(int n_phases, int stride, int klen) {
  return (255 / n_phases + 1) * stride + klen;   // floats per channel: the channel stride
}
constexpr size_t kResampleMaxLds = 64 * 1024;  // launched without raising the LDS limit
constexpr size_t resample_lds_bytes(int64_t C, int n_phases, int stride, int klen) {
  return sizeof(float) * (size_t)C * (size_t)resample_span(n_phases, stride, klen);
}

}  // namespace hfg

// mel_kernels.h — launchers of the audio front end's kernels: the log-mel framings
// (mel_kernels.hip), the resamplers (resample.hip), the PCM boundary (pcm.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hfg {

// power[b][f][k] = |sum_n w[n] x_pad[f*hop + n] e^{-2 pi i k n / n_fft}|^2
// (tcos/tsin: [n_fft][bins_pad] tables with the window folded in).
hipError_t launch_stft_power(const float* wav, int64_t B, int64_t N, int n_fft, int hop,
                             int n_bins, int n_frames, const float* tcos, const float* tsin,
                             int bins_pad, float* power, hipStream_t stream);

// mel[b][m][f] = log(sum_k fb[k][m] * power[b][f][k] + eps): log_mode 1 log10, 0 ln,
// 2 ln(v) / ln_base (a custom base, audio_processing.py:131-133)
hipError_t launch_mel_log(const float* power, int64_t B, int n_frames, int n_bins,
                          const float* fb, int n_mels, float eps, int log_mode, float ln_base,
                          float* mel, hipStream_t stream);

// Whole log-mel, FFT-based (float64 spectrum): mel[b][m][f] = log(sum_{k in band m}
// bw[k] |X_f[k]|^2 + eps) with X_f the rfft of frame f (reflect-padded, window[n] x[n] in fp32).
// n_fft a power of two >= 16; tw: n_fft complex doubles e^{-2 pi i t / n_fft}; band: per mel
// (first bin, end bin, offset into bw); fpw frames per wave (4 waves per block).
size_t logmel_fft_lds_bytes(int n_fft, int hop, int fpw, int n_mels);
hipError_t launch_logmel_fft(const float* wav, int64_t B, int64_t n_samp, int n_fft, int hop,
                             int n_frames, int fpw, const float* window, const void* tw,
                             const int* band, const float* bw, int n_mels, float eps,
                             int log_mode, float ln_base, float* mel, hipStream_t stream);

// The public HiFi-GAN release's mel (release_mel_fft), same tables and block shape as
// launch_logmel_fft (and its LDS formula): mel[b][m][f] = ln(max(sum_{k in band m} bw[k]
// sqrt(|X_f[k]|^2 + spec_eps), clip)), frame f = samples [f hop - p, f hop - p + n_fft),
// p = (n_fft - hop) / 2 (even difference), reflected at 0 and at the item's length; mel rows
// hold n_samp / hop columns.  lens (device int32 [B], or null = n_samp) is clamped into
// [0, n_samp]; item b has len / hop frames when len > p and len >= hop, else 0; columns past
// them get ln(clip); frame_lens (device int32 [B], or null) receives the frame counts.
hipError_t launch_release_mel_fft(const float* wav, int64_t B, int64_t n_samp,
                                  const int32_t* lens, int n_fft, int hop, int fpw,
                                  const float* window, const void* tw, const int* band,
                                  const float* bw, int n_mels, float spec_eps, float clip,
                                  float* mel, int32_t* frame_lens, hipStream_t stream);

// Spectral distances (spectral_distance.hip): two launches on `stream`, the distance kernel over
// (blocks of 4 fpw frames, B) and specdist_finish; nothing allocated, no atomics.  For item b,
// sums[b] = {sum |d|, sum d^2} (float64) over its compared frames and frames[b] their count.
// lens as above (null = n_samp, clamped into [0, n_samp], samples at or past it never read).
// ws: specdist_workspace_bytes(B, frames of n_samp, fpw) bytes, uninitialised.
int64_t specdist_blocks(int64_t frames, int fpw);
size_t specdist_workspace_bytes(int64_t B, int64_t frames, int fpw);
// d = (float32 mel the front end would store) - target[b][m][f], f < min(frames(len_b), T);
// target [B][n_mels][T] float32; the release framing (launch_release_mel_fft's arguments) ...
hipError_t launch_release_mel_distance(const float* wav, int64_t B, int64_t n_samp,
                                       const int32_t* lens, int n_fft, int hop, int fpw,
                                       const float* window, const void* tw, const int* band,
                                       const float* bw, int n_mels, float spec_eps, float clip,
                                       const float* target, int64_t T, double* ws, double* sums,
                                       int32_t* frames, hipStream_t stream);
// ... and the reference's (launch_logmel_fft's), item b framed as if alone: len_b / hop + 1
// frames when len_b > n_fft / 2, else 0
hipError_t launch_logmel_distance(const float* wav, int64_t B, int64_t n_samp,
                                  const int32_t* lens, int n_fft, int hop, int fpw,
                                  const float* window, const void* tw, const int* band,
                                  const float* bw, int n_mels, float eps, int log_mode,
                                  float ln_base, const float* target, int64_t T, double* ws,
                                  double* sums, int32_t* frames, hipStream_t stream);
// d = (float) ln(|X_a[k]| + eps) - (float) ln(|X_b[k]| + eps), k = 0..n_fft/2, X the rfft of the
// center=True reflect-padded frame times window (fp32 product); n_fft a power of two in
// [16, 2048]
size_t stft_distance_lds_bytes(int n_fft, int hop, int fpw);
hipError_t launch_stft_distance(const float* a, const float* b, int64_t B, int64_t n_samp,
                                const int32_t* lens, int n_fft, int hop, int fpw,
                                const float* window, const void* tw, double eps, double* ws,
                                double* sums, int32_t* frames, hipStream_t stream);

// y[b][m] = sum_k x_pad[b][(m / n_phases) * stride + k] * kern[m % n_phases][k], m < n_out,
// x_pad = x zero-padded by `width` on the left (torchaudio _apply_sinc_resample_kernel)
hipError_t launch_resample(const float* x, int64_t B, int64_t n, int64_t n_out,
                           const float* kern, int n_phases, int stride, int klen, int width,
                           float* y, hipStream_t stream);

// Ragged multi-channel resampling to mono (resample_ragged): x[B][C][n] int16 (s16) or
// float32, lens (device int32 [B], or null = n) clamped into [0, n], samples at or past an item's
// length never read.  y[b][m], m < out_len_b = ceil(n_phases len_b / stride): launch_resample's
// sum per channel on the item cropped to len_b, then ((ch_0 + ch_1) + ...) / C for C > 1; 0 for
// out_len_b <= m < n_out; out_lens (device int32 [B], or null) receives out_len_b.  kern:
// [n_phases][klen], or with tap_major [klen][n_phases].  B <= 65535, n and n_out <= INT32_MAX,
// C spans within kResampleMaxLds (lds_layout.h).
hipError_t launch_resample_ragged(const void* x, bool s16, int64_t B, int64_t C, int64_t n,
                                  const int32_t* lens, int64_t n_out, const float* kern,
                                  bool tap_major, int n_phases, int stride, int klen, int width,
                                  float* y, int32_t* out_lens, hipStream_t stream);

// The release's PCM boundary (pcm.hip), rows [B][n] of int16 (s16) or float32, B <= 65535.
// lens (device int32 [B], or null = n) is clamped into [0, n]; samples at or past an item's
// length are never read.  Plain launches: no dynamic LDS, nothing allocated.
// peak[b] = max |x| over the item (int16: |s| / 32768); peak must hold zeros on entry.
hipError_t launch_pcm_peak(const void* wav, bool s16, int64_t B, int64_t n, const int32_t* lens,
                           float* peak, hipStream_t stream);
// out[b][i] = s / 32768 (peak null) or (float)((v / d_b) * gain) in float64, d_b = peak[b], or 1
// where peak[b] is below the input type's smallest normal number; 0 for i >= len_b.
hipError_t launch_pcm_to_float(const void* wav, bool s16, int64_t B, int64_t n,
                               const int32_t* lens, const float* peak, double gain, float* out,
                               hipStream_t stream);
// offsets[B + 1]: the exclusive prefix sum of the clamped lengths.
hipError_t launch_pcm_offsets(const int32_t* lens, int64_t B, int64_t n, int64_t* offsets,
                              hipStream_t stream);
// sat16(round(x * 32768)), round toward zero or to nearest even, NaN -> 0.  offsets null:
// out[B][n], 0 for i >= len_b; else only out[offsets[b] + i], i < len_b.
hipError_t launch_pcm_from_float(const float* wav, int64_t B, int64_t n, const int32_t* lens,
                                 bool nearest, const int64_t* offsets, int16_t* out,
                                 hipStream_t stream);

}  // namespace hfg

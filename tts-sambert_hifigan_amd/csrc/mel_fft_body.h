// mel_fft_body.h — the block body of the one-launch FFT mel kernels (logmel_fft and
// release_mel_fft, mel_kernels.hip).  Device code only.
//
// Per frame (one wave): z[n] = w[2n] x[2n] + i w[2n+1] x[2n+1] (the window product in fp32,
// as torch.stft forms it), an N/2-point complex FFT in float64 (fft_f64.h) ping-ponging
// between two LDS buffers, the real-FFT split X[k] = (Z[k] + Z*[N/2-k]) / 2 -
// i e^{-2 pi i k / N} (Z[k] - Z*[N/2-k]) / 2 for k = 0..N/2, the front's spectrum of X[k], the
// mel projection over each band's nonzero bins, the front's finish.  float64 keeps the
// spectrum exact to ~1e-15 of the frame energy, so quiet bins beside loud frames keep their
// precision.  Block: 4 waves x fpw frames; the block's sample span is staged once in LDS
// (fp32) and the [n_mels][frames] tile leaves through LDS as frame-contiguous rows.
//
// A front is what the two framings differ in and nothing else: pad (the block's span starts
// at f0 hop - pad), sample(x, g) (the padded signal: reflection and what lies beyond), frames
// and n_cols (the item's valid frames, the length of a mel row), spectrum(re, im),
// finish(acc), and kPadCols / pad_val (columns at or past `frames`, and what they hold).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "fft_f64.h"
#include "kernels.h"

namespace hfg {

// torchaudio MelSpectrogram(power=2, center=True, reflect pad) -> log(mel + eps): every item
// has n_samp samples and n_frames frames (the host checks n_samp > n_fft / 2)
struct LogMelFront {
  static constexpr bool kPadCols = false;
  int pad;
  int64_t n_samp;
  int frames, n_cols;
  float eps, ln_base;
  int log_mode;
  // torch reflect: x[-i] = x[i], x[L-1+i] = x[L-1-i]; zero where one reflection does not reach
  __device__ __forceinline__ float sample(const float* __restrict__ x, int64_t g) const {
    if (g < 0) g = -g;
    if (g >= n_samp) g = 2 * (n_samp - 1) - g;
    return (g >= 0 && g < n_samp) ? x[g] : 0.f;
  }
  __device__ __forceinline__ double spectrum(double re, double im) const {
    return re * re + im * im;
  }
  __device__ __forceinline__ float finish(double acc) const {
    const double v = acc + (double)eps;
    return (float)(log_mode == 1 ? log10(v) : (log_mode == 0 ? log(v) : log(v) / (double)ln_base));
  }
};

// The HiFi-GAN release's meldataset.mel_spectrogram: pad (n_fft - hop) / 2, center=False,
// sqrt(re^2 + im^2 + spec_eps), ln(max(mel, clip)); the item has len <= n_samp samples and
// `frames` of the row's n_cols columns, the rest hold pad_val = ln(clip)
struct ReleaseMelFront {
  static constexpr bool kPadCols = true;
  int pad;
  int64_t len;
  int frames, n_cols;
  double spec_eps, clip;
  float pad_val;
  // reflected at 0 and at len; frames < len / hop reach at most pad samples past either end
  // and len > pad, so the clamp only touches samples no valid frame reads
  __device__ __forceinline__ float sample(const float* __restrict__ x, int64_t g) const {
    if (g < 0) g = -g;
    if (g >= len) g = 2 * (len - 1) - g;
    g = min(max(g, (int64_t)0), len - 1);
    return x[g];
  }
  __device__ __forceinline__ double spectrum(double re, double im) const {
    return sqrt(re * re + im * im + spec_eps);
  }
  __device__ __forceinline__ float finish(double acc) const { return (float)log(fmax(acc, clip)); }
};

// x: the block's item (blockIdx.y); mel: the whole output, indexed here (handing this function
// a row pointer instead costs registers: DESIGN.md §8)
template <class Front>
__device__ __forceinline__ void mel_fft_block(
    const Front& F, const float* __restrict__ x, int n_fft, int hop, int fpw,
    const float* __restrict__ window, const cd* __restrict__ tw, const int* __restrict__ band,
    const float* __restrict__ bw, int n_mels, float* __restrict__ mel) {
  extern __shared__ __attribute__((aligned(16))) char lds_m[];
  const int N2 = n_fft / 2;
  const int fpb = mel_fft_fpb(fpw);      // (the LDS terms: lds_layout.h)
  const int span = mel_fft_span(fpb, hop, n_fft);
  cd* const bufs = reinterpret_cast<cd*>(lds_m);                        // [4 waves][2][N2]
  float* const sig = reinterpret_cast<float*>(lds_m + mel_fft_sig_off(N2));  // [span]
  float* const mel_s = sig + mel_fft_mel_idx(span);                     // [n_mels][fpb]
  const int b = blockIdx.y;
  const int f0 = blockIdx.x * fpb;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int nf = min(fpb, F.n_cols - f0);   // columns of this block
  if constexpr (Front::kPadCols) {
    if (f0 >= F.frames) {                   // block-uniform: padding columns only
      for (int i = threadIdx.x; i < n_mels * fpb; i += 256) {
        const int m = i / fpb, fl = i - m * fpb;
        if (fl < nf) mel[((int64_t)b * n_mels + m) * F.n_cols + f0 + fl] = F.pad_val;
      }
      return;
    }
  }
  // the padded samples [f0 hop - pad, f0 hop - pad + span)
  for (int i = threadIdx.x; i < span; i += 256) sig[i] = F.sample(x, (int64_t)f0 * hop - F.pad + i);
  __syncthreads();
  cd* A = bufs + (size_t)wave * 2 * N2;
  cd* Bf = A + N2;
  for (int fi = 0; fi < fpw; ++fi) {
    const int fl = wave * fpw + fi;    // frame within the block
    if (f0 + fl >= F.frames) break;    // wave-uniform
    const float* fr = sig + fl * hop;
    for (int n = lane; n < N2; n += 64) {
      const float x0 = fr[2 * n] * window[2 * n], x1 = fr[2 * n + 1] * window[2 * n + 1];
      A[n] = {(double)x0, (double)x1};
    }
    wave_sync();
    cd* src = stockham_fft(A, Bf, N2, tw, lane);
    cd* dst = src == A ? Bf : A;
    // real-FFT split and the spectrum, k = 0..N2, into the free buffer as doubles
    double* P = reinterpret_cast<double*>(dst);
    for (int k = lane; k <= N2; k += 64) {
      const cd zk = src[k & (N2 - 1)];
      const cd zm = src[(N2 - k) & (N2 - 1)];
      const cd zc = {zm.x, -zm.y};
      const cd s_ = cadd(zk, zc), d_ = csub(zk, zc);
      const cd wd = cmul(tw[k], d_);                 // e^{-2 pi i k/N} (Z[k] - Z*[N2-k])
      const double re = 0.5 * (s_.x + wd.y), im = 0.5 * (s_.y - wd.x);  // (s - i wd) / 2
      P[k] = F.spectrum(re, im);
    }
    wave_sync();
    for (int m = lane; m < n_mels; m += 64) {
      const int lo = band[3 * m], hi = band[3 * m + 1], off = band[3 * m + 2];
      double acc = 0.0;
      for (int k = lo; k < hi; ++k) acc += (double)bw[off + k - lo] * P[k];
      mel_s[m * fpb + fl] = F.finish(acc);
    }
    wave_sync();
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n_mels * fpb; i += 256) {
    const int m = i / fpb, fl = i - m * fpb;
    if (fl < nf) {
      float v;
      if constexpr (Front::kPadCols)
        v = f0 + fl < F.frames ? mel_s[m * fpb + fl] : F.pad_val;
      else
        v = mel_s[m * fpb + fl];
      mel[((int64_t)b * n_mels + m) * F.n_cols + f0 + fl] = v;
    }
  }
}

}  // namespace hfg

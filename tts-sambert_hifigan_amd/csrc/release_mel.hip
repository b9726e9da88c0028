// release_mel.hip — the public HiFi-GAN release's mel front end (meldataset.mel_spectrogram)
// in one launch per batch: reflect pad of (n_fft - hop) / 2 a side, torch.stft(center=False,
// periodic Hann), sqrt(re^2 + im^2 + 1e-9), the librosa (Slaney) filterbank,
// ln(max(mel, 1e-5)); N samples -> N / hop frames.  Ragged batches: a per-item length.
//
// Same block shape as logmel_fft (mel_kernels.hip): 4 waves x fpw frames, the block's sample
// span staged once in LDS as fp32, one frame per wave, z[n] = w[2n] x[2n] + i w[2n+1] x[2n+1]
// (the window product in fp32, as torch.stft forms it), an N/2-point float64 Stockham FFT and
// the real-FFT split (fft_f64.h).  It differs in the framing (frame f starts at f hop - p,
// p = (n_fft - hop) / 2, indices reflected at 0 and at the item's own length), the magnitude
// spectrum, the clipped natural log, and the per-item lengths: columns at or past an item's
// frame count get log(clip), the mel of digital silence.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "fft_f64.h"
#include "kernels.h"
#include "launch.h"
#include "mel_kernels.h"

namespace hfg {

__global__ void __launch_bounds__(256)
release_mel_fft(const float* __restrict__ wav, int64_t n_samp, const int32_t* __restrict__ lens,
                int n_fft, int hop, int n_cols, int fpw, const float* __restrict__ window,
                const cd* __restrict__ tw, const int* __restrict__ band,
                const float* __restrict__ bw, int n_mels, double spec_eps, double clip,
                float pad_val, float* __restrict__ mel, int32_t* __restrict__ frame_lens) {
  extern __shared__ __attribute__((aligned(16))) char lds_r[];
  const int N2 = n_fft / 2;
  const int fpb = mel_fft_fpb(fpw);      // (the LDS terms: lds_layout.h)
  const int span = mel_fft_span(fpb, hop, n_fft);
  const int pad = (n_fft - hop) / 2;
  cd* const bufs = reinterpret_cast<cd*>(lds_r);                        // [4 waves][2][N2]
  float* const sig = reinterpret_cast<float*>(lds_r + mel_fft_sig_off(N2));  // [span]
  float* const mel_s = sig + mel_fft_mel_idx(span);                     // [n_mels][fpb]
  const int b = blockIdx.y;
  const int f0 = blockIdx.x * fpb;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  // the item's length, clamped into [0, n_samp]: whatever lens holds, every index below stays
  // inside the item's n_samp floats
  int64_t len = n_samp;
  if (lens) len = min(max((int64_t)lens[b], (int64_t)0), n_samp);
  const int frames = (len > pad && len >= hop) ? (int)min(len / hop, (int64_t)n_cols) : 0;
  if (frame_lens && blockIdx.x == 0 && threadIdx.x == 0) frame_lens[b] = frames;
  const int nf = min(fpb, n_cols - f0);   // columns of this block
  if (f0 >= frames) {                     // block-uniform: padding columns only
    for (int i = threadIdx.x; i < n_mels * fpb; i += 256) {
      const int m = i / fpb, fl = i - m * fpb;
      if (fl < nf) mel[((int64_t)b * n_mels + m) * n_cols + f0 + fl] = pad_val;
    }
    return;
  }
  const float* x = wav + (int64_t)b * n_samp;
  // samples [f0 hop - p, f0 hop - p + span), reflected at 0 and at len (torch reflect:
  // x[-i] = x[i], x[len-1+i] = x[len-1-i]); frames < len / hop reach at most p samples past
  // either end and len > p, so the clamp only touches samples no valid frame reads
  for (int i = threadIdx.x; i < span; i += 256) {
    int64_t g = (int64_t)f0 * hop - pad + i;
    if (g < 0) g = -g;
    if (g >= len) g = 2 * (len - 1) - g;
    g = min(max(g, (int64_t)0), len - 1);
    sig[i] = x[g];
  }
  __syncthreads();
  cd* A = bufs + (size_t)wave * 2 * N2;
  cd* Bf = A + N2;
  for (int fi = 0; fi < fpw; ++fi) {
    const int fl = wave * fpw + fi;  // frame within the block
    if (f0 + fl >= frames) break;    // wave-uniform
    const float* fr = sig + fl * hop;
    for (int n = lane; n < N2; n += 64) {
      const float x0 = fr[2 * n] * window[2 * n], x1 = fr[2 * n + 1] * window[2 * n + 1];
      A[n] = {(double)x0, (double)x1};
    }
    wave_sync();
    cd* src = stockham_fft(A, Bf, N2, tw, lane);
    cd* dst = src == A ? Bf : A;
    // real-FFT split and magnitude, k = 0..N2, into the free buffer as doubles
    double* P = reinterpret_cast<double*>(dst);
    for (int k = lane; k <= N2; k += 64) {
      const cd zk = src[k & (N2 - 1)];
      const cd zm = src[(N2 - k) & (N2 - 1)];
      const cd zc = {zm.x, -zm.y};
      const cd s_ = cadd(zk, zc), d_ = csub(zk, zc);
      const cd wd = cmul(tw[k], d_);                 // e^{-2 pi i k/N} (Z[k] - Z*[N2-k])
      const double re = 0.5 * (s_.x + wd.y), im = 0.5 * (s_.y - wd.x);  // (s - i wd) / 2
      P[k] = sqrt(re * re + im * im + spec_eps);
    }
    wave_sync();
    for (int m = lane; m < n_mels; m += 64) {
      const int lo = band[3 * m], hi = band[3 * m + 1], off = band[3 * m + 2];
      double acc = 0.0;
      for (int k = lo; k < hi; ++k) acc += (double)bw[off + k - lo] * P[k];
      mel_s[m * fpb + fl] = (float)log(fmax(acc, clip));
    }
    wave_sync();
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n_mels * fpb; i += 256) {
    const int m = i / fpb, fl = i - m * fpb;
    if (fl < nf)
      mel[((int64_t)b * n_mels + m) * n_cols + f0 + fl] =
          f0 + fl < frames ? mel_s[m * fpb + fl] : pad_val;
  }
}

hipError_t launch_release_mel_fft(const float* wav, int64_t B, int64_t n_samp,
                                  const int32_t* lens, int n_fft, int hop, int fpw,
                                  const float* window, const void* tw, const int* band,
                                  const float* bw, int n_mels, float spec_eps, float clip,
                                  float* mel, int32_t* frame_lens, hipStream_t stream) {
  if (n_fft < 16 || (n_fft & (n_fft - 1)) || fpw < 1 || hop < 1 || hop > n_fft ||
      ((n_fft - hop) & 1) || B < 1 || B > 65535)
    return hipErrorInvalidValue;
  const int64_t n_cols = n_samp / hop;
  if (n_cols < 1 || n_cols > INT32_MAX) return hipErrorInvalidValue;
  static auto inst = instance_of(release_mel_fft);
  auto fmt_name = [](char* s, size_t n) { snprintf(s, n, "release_mel_fft"); };
  dim3 grid((unsigned)((n_cols + 4 * fpw - 1) / (4 * fpw)), (unsigned)B);
  return launch_instance(inst, fmt_name, grid, dim3(256),
                         logmel_fft_lds_bytes(n_fft, hop, fpw, n_mels), stream, nullptr, wav,
                         n_samp, lens, n_fft, hop, (int)n_cols, fpw, window,
                         reinterpret_cast<const cd*>(tw), band, bw, n_mels, (double)spec_eps,
                         (double)clip, (float)log((double)clip), mel, frame_lens);
}

}  // namespace hfg

// mel_kernels.hip — on-device log-mel framing feeding the vocoder
// (data/audio_processing.py:98-133: torchaudio MelSpectrogram(power=2,
// center=True, reflect pad, periodic Hann) -> log10(mel + 1e-10)).
//
// stft_power_mfma: the windowed DFT of every frame as a GEMM on the fp32 matrix
//   cores: rows = 32 frames of one utterance (staged from a reflect-padded
//   signal tile in LDS), columns = frequency bins, K = n_fft samples.  The
//   twiddle tables (window folded in: w[n]cos(2 pi k n/N), w[n]sin(...)) are
//   precomputed on the host and stay L2-resident; each lane ends with Re and Im
//   of the same (frame, bin) in two accumulators and writes |X|^2.
// mel_log: mel[m][f] = log10(sum_k fb[k][m] * P[f][k] + eps), written as
//   [B][n_mels][frames], the vocoder's input layout.
// logmel_fft, release_mel_fft: the whole mel of a tile of frames in one launch, FFT-based
//   (mel_fft_body.h), in the reference's framing and in the HiFi-GAN release's.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "epilogue.h"
#include "kernels.h"
#include "launch.h"
#include "mel_fft_body.h"
#include "mel_kernels.h"

namespace hfg {

typedef float floatx16m __attribute__((ext_vector_type(16)));

// one block: 32 frames x all bins of one utterance; 4 waves split the bin tiles
__global__ void __launch_bounds__(256)
stft_power_mfma(const float* __restrict__ wav, int64_t N, int n_fft, int hop, int n_bins,
                int n_frames, const float* __restrict__ tcos, const float* __restrict__ tsin,
                int bins_pad, float* __restrict__ power) {
  extern __shared__ __attribute__((aligned(16))) float sig[];
  constexpr int FT = kStftFrames;
  const int b = blockIdx.y;
  const int f0 = blockIdx.x * FT;
  const int half_fft = n_fft / 2;
  const float* x = wav + (int64_t)b * N;
  // reflect-padded samples [f0*hop - n_fft/2, (f0+FT-1)*hop + n_fft/2)
  // stored skewed (stft_sig_idx, lds_layout.h)
  const int span = stft_span(hop, n_fft);
  for (int i = threadIdx.x; i < span; i += blockDim.x) {
    int64_t g = (int64_t)f0 * hop - half_fft + i;
    if (g < 0) g = -g;                       // torch reflect: x[-i] = x[i]
    if (g >= N) g = 2 * (N - 1) - g;         // x[N-1+i] = x[N-1-i]
    float v = 0.f;
    if (g >= 0 && g < N) v = x[g];
    sig[stft_sig_idx(i, hop)] = v;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int half = lane >> 5, col = lane & 31;
  const int n_btiles = bins_pad / 32;
  for (int bt = wave; bt < n_btiles; bt += 4) {
    floatx16m re, im;
    for (int r = 0; r < 16; ++r) {
      re[r] = 0.f;
      im[r] = 0.f;
    }
    const int bin = bt * 32 + col;
    // A[i = frame][k = n] = sig[frame*hop + n]; B[k = n][j = bin] = table[n][bin]
    const int abase = col * hop + half;  // lane's frame = col (A layout: i = lane & 31)
    const float* cb = tcos + (int64_t)half * bins_pad + bin;
    const float* sb = tsin + (int64_t)half * bins_pad + bin;
#pragma unroll 4
    for (int k = 0; k < n_fft; k += 2) {
      const int s_ = abase + k;
      const float a = sig[stft_sig_idx(s_, hop)];
      const float bc = cb[(int64_t)k * bins_pad];
      const float bs = sb[(int64_t)k * bins_pad];
      re = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bc, re, 0, 0, 0);
      im = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bs, im, 0, 0, 0);
    }
    if (bin < n_bins) {
      for (int r = 0; r < 16; ++r) {
        const int fr = f0 + acc_row(r, half);
        if (fr < n_frames)
          power[((int64_t)b * n_frames + fr) * n_bins + bin] = re[r] * re[r] + im[r] * im[r];
      }
    }
  }
}

// block: 16 frames of one utterance; power rows staged in LDS; thread = (frame, mel)
__global__ void __launch_bounds__(256)
mel_log(const float* __restrict__ power, int n_frames, int n_bins, const float* __restrict__ fb,
        int n_mels, float eps, int log_mode, float ln_base, float* __restrict__ mel) {
  extern __shared__ __attribute__((aligned(16))) float pw[];
  constexpr int FT = kMelLogFrames;
  const int b = blockIdx.y;
  const int f0 = blockIdx.x * FT;
  const int nf = min(FT, n_frames - f0);
  const float* src = power + ((int64_t)b * n_frames + f0) * n_bins;
  for (int i = threadIdx.x; i < nf * n_bins; i += blockDim.x) pw[i] = src[i];
  __syncthreads();
  for (int o = threadIdx.x; o < nf * n_mels; o += blockDim.x) {
    const int f = o / n_mels, m = o - f * n_mels;
    const float* p = pw + f * n_bins;
    float acc = 0.f;
    for (int k = 0; k < n_bins; ++k) acc = fmaf(fb[(int64_t)k * n_mels + m], p[k], acc);
    const float v = acc + eps;
    mel[((int64_t)b * n_mels + m) * n_frames + f0 + f] =
        log_mode == 1 ? log10f(v) : (log_mode == 0 ? logf(v) : logf(v) / ln_base);
  }
}

// ---------------------------------------------------------------------------------------
// logmel_fft: torchaudio MelSpectrogram(power=2, center=True) + log, one launch.  The O(N log N)
// float64 FFT replaces the O(N^2) DFT GEMM (stft_power_mfma, kept for n_fft that are not a
// power of two).
__global__ void __launch_bounds__(256)
logmel_fft(const float* __restrict__ wav, int64_t n_samp, int n_fft, int hop, int n_frames,
           int fpw, const float* __restrict__ window, const cd* __restrict__ tw,
           const int* __restrict__ band, const float* __restrict__ bw, int n_mels, float eps,
           int log_mode, float ln_base, float* __restrict__ mel) {
  const LogMelFront F{n_fft / 2, n_samp, n_frames, n_frames, eps, ln_base, log_mode};
  mel_fft_block(F, wav + (int64_t)blockIdx.y * n_samp, n_fft, hop, fpw, window, tw, band, bw,
                n_mels, mel);
}

// release_mel_fft: the public HiFi-GAN release's mel front end (meldataset.mel_spectrogram) in
// one launch per batch: reflect pad of (n_fft - hop) / 2 a side, torch.stft(center=False,
// periodic Hann), sqrt(re^2 + im^2 + 1e-9), the librosa (Slaney) filterbank,
// ln(max(mel, 1e-5)); N samples -> N / hop frames.  Ragged batches: a per-item length, indices
// reflected at 0 and at the item's own length; columns at or past an item's frame count get
// log(clip), the mel of digital silence.
__global__ void __launch_bounds__(256)
release_mel_fft(const float* __restrict__ wav, int64_t n_samp, const int32_t* __restrict__ lens,
                int n_fft, int hop, int n_cols, int fpw, const float* __restrict__ window,
                const cd* __restrict__ tw, const int* __restrict__ band,
                const float* __restrict__ bw, int n_mels, double spec_eps, double clip,
                float pad_val, float* __restrict__ mel, int32_t* __restrict__ frame_lens) {
  const int b = blockIdx.y;
  const int pad = (n_fft - hop) / 2;
  // the item's length, clamped into [0, n_samp]: whatever lens holds, every index the body
  // forms stays inside the item's n_samp floats
  int64_t len = n_samp;
  if (lens) len = min(max((int64_t)lens[b], (int64_t)0), n_samp);
  const int frames = (len > pad && len >= hop) ? (int)min(len / hop, (int64_t)n_cols) : 0;
  if (frame_lens && blockIdx.x == 0 && threadIdx.x == 0) frame_lens[b] = frames;
  const ReleaseMelFront F{pad, len, frames, n_cols, spec_eps, clip, pad_val};
  mel_fft_block(F, wav + (int64_t)b * n_samp, n_fft, hop, fpw, window, tw, band, bw, n_mels, mel);
}

static_assert(sizeof(cd) == 2 * sizeof(double), "mel_fft_lds sizes the FFT buffers");
size_t logmel_fft_lds_bytes(int n_fft, int hop, int fpw, int n_mels) {
  return mel_fft_lds_total(n_fft, hop, fpw, n_mels);
}

hipError_t launch_logmel_fft(const float* wav, int64_t B, int64_t n_samp, int n_fft, int hop,
                             int n_frames, int fpw, const float* window, const void* tw,
                             const int* band, const float* bw, int n_mels, float eps,
                             int log_mode, float ln_base, float* mel, hipStream_t stream) {
  if (n_fft < 16 || (n_fft & (n_fft - 1)) || fpw < 1) return hipErrorInvalidValue;
  static auto inst = instance_of(logmel_fft);
  auto fmt_name = [](char* s, size_t n) { snprintf(s, n, "logmel_fft"); };
  dim3 grid((n_frames + 4 * fpw - 1) / (4 * fpw), (unsigned)B);
  return launch_instance(inst, fmt_name, grid, dim3(256),
                         logmel_fft_lds_bytes(n_fft, hop, fpw, n_mels), stream, nullptr, wav,
                         n_samp, n_fft, hop, n_frames, fpw, window,
                         reinterpret_cast<const cd*>(tw), band, bw, n_mels, eps, log_mode, ln_base,
                         mel);
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

hipError_t launch_stft_power(const float* wav, int64_t B, int64_t N, int n_fft, int hop,
                             int n_bins, int n_frames, const float* tcos, const float* tsin,
                             int bins_pad, float* power, hipStream_t stream) {
  const size_t lds = stft_lds_bytes(n_fft, hop);
  if (lds > kMelDftMaxLds) return hipErrorInvalidValue;
  dim3 grid((n_frames + kStftFrames - 1) / kStftFrames, (unsigned)B);
  stft_power_mfma<<<grid, dim3(256), lds, stream>>>(wav, N, n_fft, hop, n_bins, n_frames, tcos,
                                                    tsin, bins_pad, power);
  return hipGetLastError();
}

hipError_t launch_mel_log(const float* power, int64_t B, int n_frames, int n_bins,
                          const float* fb, int n_mels, float eps, int log_mode, float ln_base,
                          float* mel, hipStream_t stream) {
  const size_t lds = mel_log_lds_bytes(n_bins);
  if (lds > kMelDftMaxLds) return hipErrorInvalidValue;
  dim3 grid((n_frames + kMelLogFrames - 1) / kMelLogFrames, (unsigned)B);
  mel_log<<<grid, dim3(256), lds, stream>>>(power, n_frames, n_bins, fb, n_mels, eps, log_mode,
                                            ln_base, mel);
  return hipGetLastError();
}

}  // namespace hfg

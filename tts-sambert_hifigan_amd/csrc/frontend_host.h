// frontend_host.h — what the audio front end's C ABI units share (defined in mel_capi.cpp):
// the error channel, the default window and filterbank arithmetic, the FFT kernels' tables.
//   mel_capi.cpp       hfg_mel_*       the reference's torchaudio log-mel
//   relmel_capi.cpp    hfg_relmel_*    the HiFi-GAN release's mel
//   resample_capi.cpp  hfg_resample_*  torchaudio Resample, fixed-length and ragged
//   pcm_capi.cpp       hfg_pcm_*       the release's PCM boundary
//   specdist_capi.cpp  hfg_*_distance, hfg_stftdist_*   spectral distances
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/hifigan_hip.h"
#include "device_guard.h"
#include "kernels.h"
#include "mel_kernels.h"

namespace hfg_host {

// the calling thread's hfg_mel_last_error text; returns code
int mfail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

// torch.stft's effective window: the periodic Hann window of win_length centred in n_fft,
// evaluated in double and rounded to fp32
std::vector<float> hann_window(int n_fft, int win_length);

// torchaudio.functional._hz_to_mel / _mel_to_hz (slaney: librosa's too, else HTK)
double hz_to_mel(double f, int slaney);
double mel_to_hz(double m, int slaney);
// out[k][m] = max(0, min(rising, falling edge of band m at freqs[k])), times 2 / (band width)
// with slaney_norm; f_pts: the n_mels + 2 band edges in Hz.  torchaudio's and librosa's
// filterbanks are this loop over grids they round differently: each caller builds its own.
void triangular_filterbank(const std::vector<double>& freqs, const std::vector<double>& f_pts,
                           int n_mels, bool slaney_norm, float* out);

// One table bound for a device slot: uploaded to `fresh`, then swapped into *dst.
struct Tbl {
  void** dst;
  const void* src;
  size_t bytes;
  void* fresh;
};

// The device tables of logmel_fft / release_mel_fft: window [n_fft] fp32, twiddles
// e^{-2 pi i t / n_fft} [n_fft] complex double, per band (first bin, end bin, offset into bw)
// and the bands' nonzero weights.
struct FftMelTables {
  float* win = nullptr;
  void* tw = nullptr;
  int* band = nullptr;
  float* bw = nullptr;
  // replaced tables: a forward in flight on any stream may still read them, so they are freed
  // by free() (or, past 256 of them, after one device sync), not by a sync per replacement
  std::vector<void*> retired;
  // Build the tables from a window [n_fft] and a filterbank [n_fft / 2 + 1][n_mels] (host,
  // fp32) and swap them in on `device` (< 0: host-only, nothing is uploaded) together with
  // `more`.  Every new table is filled before any old one is released: a failure leaves the
  // previous (complete) set in place.
  int upload(int device, int n_fft, int n_mels, const float* window, const float* fb,
             std::vector<Tbl> more = {});
  void free();
};

}  // namespace hfg_host

// The two mel handles (created in mel_capi.cpp / relmel_capi.cpp; specdist_capi.cpp runs the
// distance kernels on their tables).
struct hfg_mel_handle {
  hfg_mel_config cfg;
  int device;
  int n_bins, bins_pad;
  // DFT-GEMM path: window-folded twiddles [n_fft][bins_pad] and the filterbank [n_bins][n_mels]
  float* tcos = nullptr;
  float* tsin = nullptr;
  float* fb = nullptr;
  std::vector<float> fb_host;
  bool fft = false;  // logmel_fft (n_fft a power of two) on t's tables
  int fpw = 2;
  hfg_host::FftMelTables t;
};

struct hfg_relmel_handle {
  hfg_relmel_config cfg;  // with fmax, spec_eps and clip_val resolved
  int device;
  int fpw;
  hfg_host::FftMelTables t;
};

// specdist_capi.cpp — C ABI of the spectral distances (include/hifigan_hip_specdist.h): the
// mel of a wav against a held mel tensor on the two mel handles' own tables, and the log-STFT
// distance of two wavs on a handle of its own (one per resolution; the reference's
// compute_stft_loss, models/losses.py:625-706, runs three).  Kernels: spectral_distance.hip.
#include <cmath>

#include "frontend_host.h"

using namespace hfg_host;

struct hfg_stftdist_handle {
  hfg_stftdist_config cfg;
  double eps;               // cfg.eps, or the reference's 1e-5 (as a double) for 0
  int device;
  int fpw;
  FftMelTables t;           // the window and the twiddles (an empty one-band filterbank)
};

namespace {

// what the three forwards refuse alike; frames: of n_samples, -1 if none
int check_call(const char* what, int device, const void* p0, const void* p1, const void* ws,
               const void* sums, const void* frames_out, int64_t B, int64_t n_samples,
               int64_t frames, size_t ws_bytes, size_t ws_need) {
  if (!p0 || !p1 || !ws || !sums || !frames_out) return mfail(HFG_EINVAL, "NULL argument");
  if (device < 0) return mfail(HFG_EINVAL, "host-only %s handle", what);
  if (B <= 0 || B > 65535) return mfail(HFG_EINVAL, "B must be in [1, 65535]");
  if (frames < 1 || frames > INT32_MAX)
    return mfail(HFG_EINVAL, "%s distance: %lld samples give no frame", what,
                 (long long)n_samples);
  if (ws_bytes < ws_need)
    return mfail(HFG_EINVAL, "%s distance: workspace too small (%zu < %zu bytes)", what, ws_bytes,
                 ws_need);
  return HFG_OK;
}

int64_t mel_frames_of(const hfg_mel_handle* h, int64_t n) {
  return n > h->cfg.n_fft / 2 ? n / h->cfg.hop_length + 1 : -1;
}

}  // namespace

extern "C" {

size_t hfg_relmel_distance_workspace_bytes(const hfg_relmel_handle* h, int64_t B,
                                           int64_t n_samples) {
  if (!h || B <= 0) return 0;
  const int64_t frames = hfg_relmel_frames(h, n_samples);
  return frames < 1 ? 0 : hfg::specdist_workspace_bytes(B, frames, h->fpw);
}

int hfg_relmel_distance(hfg_relmel_handle* h, const float* wav, int64_t B, int64_t n_samples,
                        const int32_t* lengths, const float* target, int64_t target_cols,
                        void* workspace, size_t workspace_bytes, double* sums, int32_t* frames,
                        void* stream) {
  if (!h) return mfail(HFG_EINVAL, "NULL argument");
  if (int rc = check_call("release mel", h->device, wav, target, workspace, sums, frames, B,
                          n_samples, hfg_relmel_frames(h, n_samples), workspace_bytes,
                          hfg_relmel_distance_workspace_bytes(h, B, n_samples)))
    return rc;
  if (target_cols < 1 || target_cols > INT32_MAX)
    return mfail(HFG_EINVAL, "release mel distance: target_cols must be >= 1");
  DeviceGuard g(h->device);
  if (!g.ok) return mfail(HFG_ENODEV, "hipSetDevice(%d)", h->device);
  hipError_t e = hfg::launch_release_mel_distance(
      wav, B, n_samples, lengths, h->cfg.n_fft, h->cfg.hop_size, h->fpw, h->t.win, h->t.tw,
      h->t.band, h->t.bw, h->cfg.num_mels, h->cfg.spec_eps, h->cfg.clip_val, target, target_cols,
      reinterpret_cast<double*>(workspace), sums, frames, reinterpret_cast<hipStream_t>(stream));
  if (e != hipSuccess)
    return mfail(HFG_EIO, "release mel distance launch: %s", hipGetErrorString(e));
  return HFG_OK;
}

size_t hfg_mel_distance_workspace_bytes(const hfg_mel_handle* h, int64_t B, int64_t n_samples) {
  if (!h || B <= 0) return 0;
  const int64_t frames = mel_frames_of(h, n_samples);
  return frames < 1 ? 0 : hfg::specdist_workspace_bytes(B, frames, h->fpw);
}

int hfg_mel_distance(hfg_mel_handle* h, const float* wav, int64_t B, int64_t n_samples,
                     const int32_t* lengths, const float* target, int64_t target_cols,
                     void* workspace, size_t workspace_bytes, double* sums, int32_t* frames,
                     void* stream) {
  if (!h) return mfail(HFG_EINVAL, "NULL argument");
  if (!h->fft)
    return mfail(HFG_EINVAL, "mel distance: this handle runs the DFT-GEMM path (n_fft %d is not "
                 "a power of two, or MEL_DFT is forced); the distance needs the FFT path",
                 h->cfg.n_fft);
  if (int rc = check_call("mel", h->device, wav, target, workspace, sums, frames, B, n_samples,
                          mel_frames_of(h, n_samples), workspace_bytes,
                          hfg_mel_distance_workspace_bytes(h, B, n_samples)))
    return rc;
  if (target_cols < 1 || target_cols > INT32_MAX)
    return mfail(HFG_EINVAL, "mel distance: target_cols must be >= 1");
  DeviceGuard g(h->device);
  if (!g.ok) return mfail(HFG_ENODEV, "hipSetDevice(%d)", h->device);
  const hfg_mel_config& c = h->cfg;
  const int log_mode = c.log_base == 10 ? 1 : (c.log_base == 0 ? 0 : 2);
  const float ln_base = std::log(c.log_base_value);   // as hfg_mel_forward
  hipError_t e = hfg::launch_logmel_distance(
      wav, B, n_samples, lengths, c.n_fft, c.hop_length, h->fpw, h->t.win, h->t.tw, h->t.band,
      h->t.bw, c.n_mels, c.log_eps, log_mode, ln_base, target, target_cols,
      reinterpret_cast<double*>(workspace), sums, frames, reinterpret_cast<hipStream_t>(stream));
  if (e != hipSuccess) return mfail(HFG_EIO, "mel distance launch: %s", hipGetErrorString(e));
  return HFG_OK;
}

int hfg_stftdist_create(const hfg_stftdist_config* cfg, int device, hfg_stftdist_handle** out) {
  if (!cfg || !out) return mfail(HFG_EINVAL, "NULL argument");
  *out = nullptr;
  hfg_stftdist_config c = *cfg;
  if (c.n_fft < 16 || (c.n_fft & (c.n_fft - 1)))
    return mfail(HFG_EINVAL, "stft distance: n_fft must be a power of two >= 16, got %d", c.n_fft);
  if (c.hop_length < 1) return mfail(HFG_EINVAL, "stft distance: hop_length must be >= 1");
  if (c.win_length < 1 || c.win_length > c.n_fft)
    return mfail(HFG_EINVAL, "stft distance: win_length must be in [1, n_fft]");
  const double eps = c.eps == 0.f ? 1e-5 : (double)c.eps;
  if (!(eps > 0.0)) return mfail(HFG_EINVAL, "stft distance: eps must be > 0");
  const int fpw = c.n_fft <= 1024 ? 2 : 1;
  if (c.n_fft > 2048 ||
      hfg::stft_distance_lds_bytes(c.n_fft, c.hop_length, fpw) > hfg::kMaxLdsBytes)
    return mfail(HFG_EINVAL, "stft distance: n_fft %d / hop_length %d too large for the LDS "
                 "frame tile", c.n_fft, c.hop_length);
  auto* h = new (std::nothrow) hfg_stftdist_handle();
  if (!h) return mfail(HFG_ENOMEM, "host alloc");
  h->cfg = c;
  h->eps = eps;
  h->device = device;
  h->fpw = fpw;
  int rc = hfg_stftdist_set_window(h, hann_window(c.n_fft, c.win_length).data());
  if (rc) {
    hfg_stftdist_destroy(h);
    return rc;
  }
  *out = h;
  return HFG_OK;
}

int hfg_stftdist_set_window(hfg_stftdist_handle* h, const float* window) {
  if (!h || !window) return mfail(HFG_EINVAL, "NULL argument");
  const std::vector<float> no_band((size_t)h->cfg.n_fft / 2 + 1, 0.f);
  return h->t.upload(h->device, h->cfg.n_fft, 1, window, no_band.data());
}

void hfg_stftdist_destroy(hfg_stftdist_handle* h) {
  if (!h) return;
  h->t.free();
  delete h;
}

int64_t hfg_stftdist_frames(const hfg_stftdist_handle* h, int64_t n_samples) {
  if (!h || n_samples <= h->cfg.n_fft / 2) return -1;
  return n_samples / h->cfg.hop_length + 1;
}

size_t hfg_stftdist_workspace_bytes(const hfg_stftdist_handle* h, int64_t B, int64_t n_samples) {
  if (!h || B <= 0) return 0;
  const int64_t frames = hfg_stftdist_frames(h, n_samples);
  return frames < 1 ? 0 : hfg::specdist_workspace_bytes(B, frames, h->fpw);
}

int hfg_stftdist_forward(hfg_stftdist_handle* h, const float* a, const float* b, int64_t B,
                         int64_t n_samples, const int32_t* lengths, void* workspace,
                         size_t workspace_bytes, double* sums, int32_t* frames, void* stream) {
  if (!h) return mfail(HFG_EINVAL, "NULL argument");
  if (int rc = check_call("stft", h->device, a, b, workspace, sums, frames, B, n_samples,
                          hfg_stftdist_frames(h, n_samples), workspace_bytes,
                          hfg_stftdist_workspace_bytes(h, B, n_samples)))
    return rc;
  DeviceGuard g(h->device);
  if (!g.ok) return mfail(HFG_ENODEV, "hipSetDevice(%d)", h->device);
  hipError_t e = hfg::launch_stft_distance(
      a, b, B, n_samples, lengths, h->cfg.n_fft, h->cfg.hop_length, h->fpw, h->t.win, h->t.tw,
      h->eps, reinterpret_cast<double*>(workspace), sums, frames,
      reinterpret_cast<hipStream_t>(stream));
  if (e != hipSuccess) return mfail(HFG_EIO, "stft distance launch: %s", hipGetErrorString(e));
  return HFG_OK;
}

}  // extern "C"

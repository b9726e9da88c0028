// relmel_capi.cpp — C ABI of the public HiFi-GAN release's mel front end
// (include/hifigan_hip_relmel.h).  meldataset.mel_spectrogram: reflect pad (n_fft - hop) / 2,
// torch.stft(center=False), sqrt(re^2 + im^2 + 1e-9), librosa.filters.mel, ln(max(mel, 1e-5));
// one launch of release_mel_fft (mel_kernels.hip), per-item lengths.
#include "../../include/hifigan_hip_relmel.h"
#include "frontend_host.h"

using namespace hfg_host;

namespace {

// librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax) (htk=False, norm="slaney") in double:
// out[k][m], k < n_fft/2 + 1
void librosa_mel(const hfg_relmel_config* c, float* out) {
  const int n_bins = c->n_fft / 2 + 1, n_mels = c->num_mels;
  std::vector<double> fftfreqs(n_bins), mel_f(n_mels + 2);
  const double fstep = (0.5 * c->sampling_rate) / (double)(n_bins - 1);
  for (int k = 0; k < n_bins; ++k) fftfreqs[k] = k * fstep;
  fftfreqs[n_bins - 1] = 0.5 * c->sampling_rate;
  const double m_min = hz_to_mel(c->fmin, 1), m_max = hz_to_mel(c->fmax, 1);
  const double mstep = (m_max - m_min) / (double)(n_mels + 1);
  for (int i = 0; i < n_mels + 2; ++i)
    mel_f[i] = mel_to_hz(i == n_mels + 1 ? m_max : m_min + i * mstep, 1);
  triangular_filterbank(fftfreqs, mel_f, n_mels, true, out);
}

}  // namespace

extern "C" {

int hfg_relmel_create(const hfg_relmel_config* cfg, int device, hfg_relmel_handle** out) {
  if (!cfg || !out) return mfail(HFG_EINVAL, "NULL argument");
  *out = nullptr;
  hfg_relmel_config c = *cfg;
  if (c.sampling_rate <= 0 || c.n_fft <= 0 || c.hop_size <= 0 || c.win_size <= 0 ||
      c.num_mels <= 0)
    return mfail(HFG_EINVAL, "invalid release mel configuration");
  if (c.n_fft < 16 || (c.n_fft & (c.n_fft - 1)))
    return mfail(HFG_EINVAL, "release mel: n_fft must be a power of two >= 16, got %d", c.n_fft);
  if (c.hop_size > c.n_fft || ((c.n_fft - c.hop_size) & 1))
    return mfail(HFG_EINVAL, "release mel: n_fft - hop_size must be even and >= 0 (n_fft %d, "
                 "hop_size %d)", c.n_fft, c.hop_size);
  if (c.win_size > c.n_fft) return mfail(HFG_EINVAL, "release mel: win_size > n_fft");
  if (!(c.fmax > 0.f)) c.fmax = 0.5f * (float)c.sampling_rate;  // the release's null
  if (!(c.fmin >= 0.f) || !(c.fmax > c.fmin))
    return mfail(HFG_EINVAL, "release mel: need 0 <= fmin < fmax");
  if (c.spec_eps == 0.f) c.spec_eps = 1e-9f;
  if (c.clip_val == 0.f) c.clip_val = 1e-5f;
  if (!(c.spec_eps > 0.f) || !(c.clip_val > 0.f))
    return mfail(HFG_EINVAL, "release mel: spec_eps and clip_val must be > 0");
  const int fpw = c.n_fft <= 1024 ? 2 : 1;
  if (hfg::logmel_fft_lds_bytes(c.n_fft, c.hop_size, fpw, c.num_mels) > hfg::kMaxLdsBytes)
    return mfail(HFG_EINVAL, "release mel: n_fft %d / num_mels %d too large for the LDS frame "
                 "tile", c.n_fft, c.num_mels);
  auto* h = new (std::nothrow) hfg_relmel_handle();
  if (!h) return mfail(HFG_ENOMEM, "host alloc");
  h->cfg = c;
  h->device = device;
  h->fpw = fpw;
  std::vector<float> fb_h((size_t)(c.n_fft / 2 + 1) * c.num_mels);
  librosa_mel(&c, fb_h.data());
  int rc = hfg_relmel_set_tables(h, hann_window(c.n_fft, c.win_size).data(), fb_h.data());
  if (rc) {
    hfg_relmel_destroy(h);
    return rc;
  }
  *out = h;
  return HFG_OK;
}

void hfg_relmel_destroy(hfg_relmel_handle* h) {
  if (!h) return;
  h->t.free();
  delete h;
}

int hfg_relmel_set_tables(hfg_relmel_handle* h, const float* window, const float* fb) {
  if (!h || !window || !fb) return mfail(HFG_EINVAL, "NULL argument");
  return h->t.upload(h->device, h->cfg.n_fft, h->cfg.num_mels, window, fb);
}

int64_t hfg_relmel_frames(const hfg_relmel_handle* h, int64_t n_samples) {
  if (!h) return -1;
  const int64_t pad = (h->cfg.n_fft - h->cfg.hop_size) / 2;
  if (n_samples <= pad || n_samples < h->cfg.hop_size) return -1;
  return n_samples / h->cfg.hop_size;
}

int hfg_relmel_forward(hfg_relmel_handle* h, const float* wav, int64_t B, int64_t n_samples,
                       const int32_t* lengths, float* mel, int32_t* frame_lengths, void* stream) {
  if (!h || !wav || !mel) return mfail(HFG_EINVAL, "NULL argument");
  if (h->device < 0) return mfail(HFG_EINVAL, "host-only release mel handle");
  if (B <= 0 || B > 65535) return mfail(HFG_EINVAL, "B must be in [1, 65535]");
  const int64_t n_frames = hfg_relmel_frames(h, n_samples);
  if (n_frames < 1 || n_frames > INT32_MAX)
    return mfail(HFG_EINVAL, "release mel: %lld samples give no frame (need more than "
                 "(n_fft - hop) / 2 = %d and at least hop = %d)", (long long)n_samples,
                 (h->cfg.n_fft - h->cfg.hop_size) / 2, h->cfg.hop_size);
  DeviceGuard g(h->device);
  if (!g.ok) return mfail(HFG_ENODEV, "hipSetDevice(%d)", h->device);
  hipError_t e = hfg::launch_release_mel_fft(
      wav, B, n_samples, lengths, h->cfg.n_fft, h->cfg.hop_size, h->fpw, h->t.win, h->t.tw,
      h->t.band, h->t.bw, h->cfg.num_mels, h->cfg.spec_eps, h->cfg.clip_val, mel, frame_lengths,
      reinterpret_cast<hipStream_t>(stream));
  if (e != hipSuccess) return mfail(HFG_EIO, "release mel launch: %s", hipGetErrorString(e));
  return HFG_OK;
}

}  // extern "C"

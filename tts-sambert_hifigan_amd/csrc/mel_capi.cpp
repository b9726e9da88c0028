// mel_capi.cpp — C ABI of the on-device log-mel framing (include/hifigan_hip.h,
// "mel" section): the host builds the windowed DFT tables and the mel filterbank
// once per handle, forward is one or two async launches on the caller's stream.  Also defines
// what the front end's units share (frontend_host.h).
//
// Restates torchaudio.transforms.MelSpectrogram as configured at
// data/audio_processing.py:99-110 (n_fft 1024, hop 256, win 1024, 80 mels,
// 0-8000 Hz, slaney scale + slaney norm, power 2, center=True, reflect pad,
// periodic Hann) and the log at :123-133.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <string>

#include "../../include/hifigan_hip_inspect.h"
#include "frontend_host.h"

namespace hfg_host {

namespace {
thread_local std::string g_mel_err;
constexpr double kTwoPi = 6.283185307179586476925286766559;
}  // namespace

int mfail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_mel_err = buf;
  return code;
}

std::vector<float> hann_window(int n_fft, int win_length) {
  const int left = (n_fft - win_length) / 2;
  std::vector<float> w(n_fft, 0.f);
  for (int n = 0; n < n_fft; ++n) {
    const int wi = n - left;
    if (wi >= 0 && wi < win_length) w[n] = (float)(0.5 - 0.5 * std::cos(kTwoPi * wi / win_length));
  }
  return w;
}

double hz_to_mel(double f, int slaney) {
  if (!slaney) return 2595.0 * std::log10(1.0 + f / 700.0);
  const double f_sp = 200.0 / 3.0, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp;
  const double logstep = std::log(6.4) / 27.0;
  return f >= min_log_hz ? min_log_mel + std::log(f / min_log_hz) / logstep : f / f_sp;
}
double mel_to_hz(double m, int slaney) {
  if (!slaney) return 700.0 * (std::pow(10.0, m / 2595.0) - 1.0);
  const double f_sp = 200.0 / 3.0, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp;
  const double logstep = std::log(6.4) / 27.0;
  return m >= min_log_mel ? min_log_hz * std::exp(logstep * (m - min_log_mel)) : f_sp * m;
}

void triangular_filterbank(const std::vector<double>& freqs, const std::vector<double>& f_pts,
                           int n_mels, bool slaney_norm, float* out) {
  for (size_t k = 0; k < freqs.size(); ++k)
    for (int m = 0; m < n_mels; ++m) {
      const double down = -(f_pts[m] - freqs[k]) / (f_pts[m + 1] - f_pts[m]);
      const double up = (f_pts[m + 2] - freqs[k]) / (f_pts[m + 2] - f_pts[m + 1]);
      double v = std::fmax(0.0, std::fmin(down, up));
      if (slaney_norm) v *= 2.0 / (f_pts[m + 2] - f_pts[m]);
      out[k * n_mels + m] = (float)v;
    }
}

int FftMelTables::upload(int device, int n_fft, int n_mels, const float* window, const float* fb,
                         std::vector<Tbl> tbls) {
  if (device < 0) return HFG_OK;
  const int n_bins = n_fft / 2 + 1;
  std::vector<double> tw_h(2 * (size_t)n_fft);
  for (int i = 0; i < n_fft; ++i) {
    tw_h[2 * i] = std::cos(kTwoPi * i / n_fft);
    tw_h[2 * i + 1] = -std::sin(kTwoPi * i / n_fft);
  }
  std::vector<int> band_h(3 * (size_t)n_mels);
  std::vector<float> bw_h;
  for (int m = 0; m < n_mels; ++m) {
    int lo = n_bins, hi = 0;
    for (int k = 0; k < n_bins; ++k)
      if (fb[(size_t)k * n_mels + m] != 0.f) {
        lo = std::min(lo, k);
        hi = k + 1;
      }
    if (hi <= lo) lo = hi = 0;
    band_h[3 * m] = lo;
    band_h[3 * m + 1] = hi;
    band_h[3 * m + 2] = (int)bw_h.size();
    for (int k = lo; k < hi; ++k) bw_h.push_back(fb[(size_t)k * n_mels + m]);
  }
  if (bw_h.empty()) bw_h.push_back(0.f);
  tbls.push_back({reinterpret_cast<void**>(&win), window, (size_t)n_fft * 4, nullptr});
  tbls.push_back({&tw, tw_h.data(), tw_h.size() * 8, nullptr});
  tbls.push_back({reinterpret_cast<void**>(&band), band_h.data(), band_h.size() * 4, nullptr});
  tbls.push_back({reinterpret_cast<void**>(&bw), bw_h.data(), bw_h.size() * 4, nullptr});

  DeviceGuard g(device);
  if (!g.ok) return mfail(HFG_ENODEV, "hipSetDevice(%d)", device);
  bool ok = true;
  for (auto& t : tbls) {
    ok = hipMalloc(&t.fresh, t.bytes) == hipSuccess &&
         hipMemcpy(t.fresh, t.src, t.bytes, hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) break;
  }
  constexpr size_t kMaxRetired = 256;
  if (ok && retired.size() + tbls.size() > kMaxRetired) {
    // rare (hundreds of replacements): one sync retires every old table at once
    ok = hipDeviceSynchronize() == hipSuccess;
    if (ok) {
      for (void* p : retired) (void)hipFree(p);
      retired.clear();
    }
  }
  for (auto& t : tbls) {
    if (ok) {
      if (*t.dst) retired.push_back(*t.dst);
      *t.dst = t.fresh;
    } else if (t.fresh) {
      (void)hipFree(t.fresh);
    }
  }
  return ok ? HFG_OK : mfail(HFG_ENOMEM, "mel tables: device allocation / copy failed");
}

void FftMelTables::free() {
  for (void* p : {(void*)win, tw, (void*)band, (void*)bw})
    if (p) (void)hipFree(p);
  for (void* p : retired) (void)hipFree(p);
}

}  // namespace hfg_host

using namespace hfg_host;

namespace {

// Build and upload every device table from a window [n_fft] and a filterbank
// [n_bins][n_mels] (host, fp32): the DFT-GEMM path's windowed twiddles beside the FFT path's.
int upload_tables(hfg_mel_handle* h, const float* win, const float* fb) {
  const int N = h->cfg.n_fft, n_mels = h->cfg.n_mels;
  if (fb != h->fb_host.data()) h->fb_host.assign(fb, fb + (size_t)h->n_bins * n_mels);
  std::vector<float> tc, ts;
  std::vector<Tbl> dft;
  if (!h->fft && h->device >= 0) {
    tc.assign((size_t)N * h->bins_pad, 0.f);
    ts.assign((size_t)N * h->bins_pad, 0.f);
    for (int n = 0; n < N; ++n)
      for (int k = 0; k < h->n_bins; ++k) {
        const double ang = kTwoPi * (double)(((long long)k * n) % N) / N;
        tc[(size_t)n * h->bins_pad + k] = (float)((double)win[n] * std::cos(ang));
        ts[(size_t)n * h->bins_pad + k] = (float)(-(double)win[n] * std::sin(ang));
      }
    dft.push_back({reinterpret_cast<void**>(&h->tcos), tc.data(), tc.size() * 4, nullptr});
    dft.push_back({reinterpret_cast<void**>(&h->tsin), ts.data(), ts.size() * 4, nullptr});
    dft.push_back({reinterpret_cast<void**>(&h->fb), fb, h->fb_host.size() * 4, nullptr});
  }
  return h->t.upload(h->device, N, n_mels, win, fb, dft);
}

}  // namespace

extern "C" {

const char* hfg_mel_last_error(void) { return g_mel_err.c_str(); }

int hfg_mel_filterbank(const hfg_mel_config* c, float* out) {
  // torchaudio.functional.melscale_fbanks(n_freqs, f_min, f_max, n_mels, sr, norm, mel_scale)
  const int n_freqs = c->n_fft / 2 + 1, n_mels = c->n_mels;
  const int slaney = c->mel_scale == 0;
  std::vector<double> all_freqs(n_freqs), f_pts(n_mels + 2);
  for (int i = 0; i < n_freqs; ++i)
    all_freqs[i] = (double)(c->sample_rate / 2) * i / (double)(n_freqs - 1);
  const double m_min = hz_to_mel(c->f_min, slaney), m_max = hz_to_mel(c->f_max, slaney);
  for (int i = 0; i < n_mels + 2; ++i)
    f_pts[i] = mel_to_hz(m_min + (m_max - m_min) * i / (double)(n_mels + 1), slaney);
  triangular_filterbank(all_freqs, f_pts, n_mels, c->norm == 1, out);
  return HFG_OK;
}

int hfg_mel_create(const hfg_mel_config* c, int device, hfg_mel_handle** out) {
  if (!c || !out) return mfail(HFG_EINVAL, "NULL argument");
  *out = nullptr;
  if (c->n_fft <= 0 || (c->n_fft & 1) || c->hop_length <= 0 || c->win_length <= 0 ||
      c->win_length > c->n_fft || c->n_mels <= 0 || c->sample_rate <= 0 ||
      !(c->f_max > c->f_min) || c->f_min < 0)
    return mfail(HFG_EINVAL, "invalid mel configuration");
  if (c->mel_scale != 0 && c->mel_scale != 1) return mfail(HFG_EINVAL, "mel_scale 0|1");
  if (c->norm != 0 && c->norm != 1) return mfail(HFG_EINVAL, "norm 0|1");
  if (c->log_base != 10 && c->log_base != 0 && c->log_base != 1)
    return mfail(HFG_EINVAL, "log_base: 10 (log10), 0 (ln) or 1 (custom base)");
  if (c->log_base == 1 && !(c->log_base_value > 0.f && c->log_base_value != 1.f))
    return mfail(HFG_EINVAL, "custom log base must be > 0 and != 1");
  const int N = c->n_fft;
  const int fpw = N <= 1024 ? 2 : 1;
  int md = 0;  // 1: the DFT-GEMM path (A/B and fallback tests: hfg_debug_schedule_set)
  hfg_debug_schedule_get("MEL_DFT", &md);
  const bool fft = (N & (N - 1)) == 0 && N >= 16 && md == 0 &&
                   hfg::logmel_fft_lds_bytes(N, c->hop_length, fpw, c->n_mels) <= hfg::kMaxLdsBytes;
  // the DFT-GEMM path is the fallback for n_fft that are not a power of two
  if (!fft && !hfg::mel_dft_fits(N, c->hop_length))
    return mfail(HFG_EINVAL, "n_fft / hop too large for the LDS frame tiles");
  auto* h = new (std::nothrow) hfg_mel_handle();
  if (!h) return mfail(HFG_ENOMEM, "host alloc");
  h->cfg = *c;
  h->device = device;
  h->n_bins = N / 2 + 1;
  h->bins_pad = (h->n_bins + 31) / 32 * 32;
  h->fpw = fpw;
  h->fft = fft;
  // default tables: torch.stft's window and torchaudio's filterbank, both evaluated in double
  // and rounded to fp32 (the Python layer replaces them by the float32-evaluated torch tables,
  // hfg_mel_set_tables)
  h->fb_host.resize((size_t)h->n_bins * c->n_mels);
  hfg_mel_filterbank(c, h->fb_host.data());
  int rc = upload_tables(h, hann_window(N, c->win_length).data(), h->fb_host.data());
  if (rc) {
    hfg_mel_destroy(h);
    return rc;
  }
  *out = h;
  return HFG_OK;
}

void hfg_mel_destroy(hfg_mel_handle* h) {
  if (!h) return;
  if (h->tcos) (void)hipFree(h->tcos);
  if (h->tsin) (void)hipFree(h->tsin);
  if (h->fb) (void)hipFree(h->fb);
  h->t.free();
  delete h;
}

int hfg_mel_set_tables(hfg_mel_handle* h, const float* window, const float* fb) {
  if (!h || !window || !fb) return mfail(HFG_EINVAL, "NULL argument");
  return upload_tables(h, window, fb);
}

int64_t hfg_mel_frames(const hfg_mel_handle* h, int64_t n_samples) {
  if (!h || n_samples <= 0) return -1;
  return n_samples / h->cfg.hop_length + 1;  // center=True
}

size_t hfg_mel_workspace_bytes(const hfg_mel_handle* h, int64_t B, int64_t n_samples) {
  if (!h || B <= 0 || n_samples <= 0) return 0;
  // the one-launch FFT path keeps its spectra in LDS: no workspace (a token 256 B, so callers
  // that allocate what this returns hold a valid pointer)
  if (h->fft) return 256;
  return sizeof(float) * (size_t)B * (size_t)hfg_mel_frames(h, n_samples) * (size_t)h->n_bins;
}

int hfg_mel_forward(hfg_mel_handle* h, const float* wav, int64_t B, int64_t n_samples, float* mel,
                    void* workspace, size_t workspace_bytes, void* stream) {
  if (!h || !wav || !mel || (!workspace && !h->fft)) return mfail(HFG_EINVAL, "NULL argument");
  if (h->device < 0) return mfail(HFG_EINVAL, "host-only mel handle");
  if (B <= 0) return mfail(HFG_EINVAL, "B must be > 0");
  if (n_samples <= h->cfg.n_fft / 2)
    return mfail(HFG_EINVAL, "reflect padding needs more than n_fft/2 = %d samples",
                 h->cfg.n_fft / 2);
  if (workspace_bytes < hfg_mel_workspace_bytes(h, B, n_samples))
    return mfail(HFG_EINVAL, "workspace too small");
  const int n_frames = (int)hfg_mel_frames(h, n_samples);
  DeviceGuard g(h->device);
  if (!g.ok) return mfail(HFG_ENODEV, "hipSetDevice(%d)", h->device);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const hfg_mel_config& c = h->cfg;
  const int log_mode = c.log_base == 10 ? 1 : (c.log_base == 0 ? 0 : 2);
  // torch.log(torch.tensor(log_base)): a float32 log of the base
  const float ln_base = std::log(c.log_base_value);
  hipError_t e;
  if (h->fft) {
    e = hfg::launch_logmel_fft(wav, B, n_samples, c.n_fft, c.hop_length, n_frames, h->fpw,
                               h->t.win, h->t.tw, h->t.band, h->t.bw, c.n_mels, c.log_eps,
                               log_mode, ln_base, mel, s);
  } else {
    float* power = reinterpret_cast<float*>(workspace);
    e = hfg::launch_stft_power(wav, B, n_samples, c.n_fft, c.hop_length, h->n_bins, n_frames,
                               h->tcos, h->tsin, h->bins_pad, power, s);
    if (e == hipSuccess)
      e = hfg::launch_mel_log(power, B, n_frames, h->n_bins, h->fb, c.n_mels, c.log_eps, log_mode,
                              ln_base, mel, s);
  }
  if (e != hipSuccess) return mfail(HFG_EIO, "mel launch: %s", hipGetErrorString(e));
  return HFG_OK;
}

}  // extern "C"

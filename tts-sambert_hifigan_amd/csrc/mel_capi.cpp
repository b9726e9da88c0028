// mel_capi.cpp — C ABI of the on-device log-mel framing (include/hifigan_hip.h,
// "mel" section): the host builds the windowed DFT tables and the mel filterbank
// once per handle, forward is two async launches on the caller's stream.
//
// Restates torchaudio.transforms.MelSpectrogram as configured at
// data/audio_processing.py:99-110 (n_fft 1024, hop 256, win 1024, 80 mels,
// 0-8000 Hz, slaney scale + slaney norm, power 2, center=True, reflect pad,
// periodic Hann) and the log at :123-133.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/hifigan_hip.h"
#include "../../include/hifigan_hip_inspect.h"
#include "kernels.h"
#include "mel_kernels.h"

namespace {

thread_local std::string g_mel_err;

int mfail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_mel_err = buf;
  return code;
}

// torchaudio.functional._hz_to_mel / _mel_to_hz
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

}  // namespace

struct hfg_mel_handle {
  hfg_mel_config cfg;
  int device;
  int n_bins, bins_pad;
  float* tcos = nullptr;  // [n_fft][bins_pad]
  float* tsin = nullptr;
  float* fb = nullptr;    // [n_bins][n_mels]
  std::vector<float> fb_host;
  // FFT path (logmel_fft, n_fft a power of two): window [n_fft] fp32, twiddles [n_fft]
  // complex double, per-band (first bin, end bin, offset) and the bands' nonzero weights
  bool fft = false;
  int fpw = 2;
  float* win = nullptr;
  void* tw = nullptr;
  int* band = nullptr;
  float* bw = nullptr;
  // tables replaced by hfg_mel_set_tables: a forward still in flight on any stream may read
  // them, so they are freed at destroy (or, past kMaxRetired, after one device sync) instead of
  // syncing the device on every replacement
  std::vector<void*> retired;
};

namespace {

// Host side of the FFT kernels' tables (logmel_fft, release_mel_fft): e^{-2 pi i t / N} in
// float64 and, from a filterbank [n_bins][n_mels], each band's (first bin, end bin, offset)
// and its nonzero weights.
struct FftTables {
  std::vector<double> tw;
  std::vector<int> band;
  std::vector<float> bw;
};
FftTables fft_host_tables(int N, int n_bins, int n_mels, const float* fb) {
  const double two_pi = 6.283185307179586476925286766559;
  FftTables t;
  t.tw.resize(2 * (size_t)N);
  for (int i = 0; i < N; ++i) {
    t.tw[2 * i] = std::cos(two_pi * i / N);
    t.tw[2 * i + 1] = -std::sin(two_pi * i / N);
  }
  t.band.resize(3 * (size_t)n_mels);
  for (int m = 0; m < n_mels; ++m) {
    int lo = n_bins, hi = 0;
    for (int k = 0; k < n_bins; ++k)
      if (fb[(size_t)k * n_mels + m] != 0.f) {
        lo = std::min(lo, k);
        hi = k + 1;
      }
    if (hi <= lo) lo = hi = 0;
    t.band[3 * m] = lo;
    t.band[3 * m + 1] = hi;
    t.band[3 * m + 2] = (int)t.bw.size();
    for (int k = lo; k < hi; ++k) t.bw.push_back(fb[(size_t)k * n_mels + m]);
  }
  if (t.bw.empty()) t.bw.push_back(0.f);
  return t;
}

struct Tbl {
  void** dst;
  const void* src;
  size_t bytes;
  void* fresh;
};
// Upload every table of `tbls` to `device` and swap it into its handle slot.  Every new
// table is allocated and filled before any old one is released: a failure leaves the
// handle's previous (complete) tables in place.  A forward still in flight may
// read an old table, so those go to `retired` (freed at destroy).
int swap_tables(int device, std::vector<Tbl>& tbls, std::vector<void*>& retired) {
  int prev = -1;
  (void)hipGetDevice(&prev);
  if (hipSetDevice(device) != hipSuccess) return mfail(HFG_ENODEV, "hipSetDevice(%d)", device);
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
  if (prev >= 0) (void)hipSetDevice(prev);
  return ok ? HFG_OK : mfail(HFG_ENOMEM, "mel tables: device allocation / copy failed");
}

// Build and upload every device table from a window [n_fft] and a filterbank
// [n_bins][n_mels] (host, fp32): the DFT-GEMM path's windowed twiddles, the FFT path's
// window, e^{-2 pi i t / N} (float64) and each band's nonzero bins.
int upload_tables(hfg_mel_handle* h, const float* win, const float* fb) {
  const hfg_mel_config* c = &h->cfg;
  const int N = c->n_fft, n_mels = c->n_mels;
  const double two_pi = 6.283185307179586476925286766559;
  if (fb != h->fb_host.data()) h->fb_host.assign(fb, fb + (size_t)h->n_bins * n_mels);
  std::vector<float> tc, ts;
  if (!h->fft) {
    tc.assign((size_t)N * h->bins_pad, 0.f);
    ts.assign((size_t)N * h->bins_pad, 0.f);
    for (int n = 0; n < N; ++n)
      for (int k = 0; k < h->n_bins; ++k) {
        const double ang = two_pi * (double)(((long long)k * n) % N) / N;
        tc[(size_t)n * h->bins_pad + k] = (float)((double)win[n] * std::cos(ang));
        ts[(size_t)n * h->bins_pad + k] = (float)(-(double)win[n] * std::sin(ang));
      }
  }
  const FftTables ft = fft_host_tables(N, h->n_bins, n_mels, fb);
  if (h->device < 0) return HFG_OK;
  std::vector<Tbl> tbls;
  if (!h->fft) {
    tbls.push_back({reinterpret_cast<void**>(&h->tcos), tc.data(), tc.size() * 4, nullptr});
    tbls.push_back({reinterpret_cast<void**>(&h->tsin), ts.data(), ts.size() * 4, nullptr});
    tbls.push_back({reinterpret_cast<void**>(&h->fb), fb, h->fb_host.size() * 4, nullptr});
  }
  tbls.push_back({reinterpret_cast<void**>(&h->win), win, (size_t)N * 4, nullptr});
  tbls.push_back({&h->tw, ft.tw.data(), ft.tw.size() * 8, nullptr});
  tbls.push_back({reinterpret_cast<void**>(&h->band), ft.band.data(), ft.band.size() * 4, nullptr});
  tbls.push_back({reinterpret_cast<void**>(&h->bw), ft.bw.data(), ft.bw.size() * 4, nullptr});
  return swap_tables(h->device, tbls, h->retired);
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
  for (int k = 0; k < n_freqs; ++k)
    for (int m = 0; m < n_mels; ++m) {
      const double down = -(f_pts[m] - all_freqs[k]) / (f_pts[m + 1] - f_pts[m]);
      const double up = (f_pts[m + 2] - all_freqs[k]) / (f_pts[m + 2] - f_pts[m + 1]);
      double v = std::fmax(0.0, std::fmin(down, up));
      if (c->norm == 1) v *= 2.0 / (f_pts[m + 2] - f_pts[m]);
      out[(size_t)k * n_mels + m] = (float)v;
    }
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
  // the DFT-GEMM path's LDS tiles (the fallback for n_fft that are not a power of two)
  const bool dft_fits = (size_t)(31 * c->hop_length + c->n_fft) * 4 * 33 / 32 <= 64 * 1024 &&
                        (size_t)16 * (c->n_fft / 2 + 1) * 4 <= 64 * 1024;
  auto* h = new (std::nothrow) hfg_mel_handle();
  if (!h) return mfail(HFG_ENOMEM, "host alloc");
  h->cfg = *c;
  h->device = device;
  h->n_bins = c->n_fft / 2 + 1;
  h->bins_pad = (h->n_bins + 31) / 32 * 32;
  // default tables: the periodic Hann window of win_length centred in n_fft (torch.stft)
  // and torchaudio's filterbank, both evaluated in double and rounded to fp32 (the Python
  // layer replaces them by the float32-evaluated torch tables, hfg_mel_set_tables)
  const int N = c->n_fft, W = c->win_length, left = (N - W) / 2;
  const double two_pi = 6.283185307179586476925286766559;
  std::vector<float> win_h(N, 0.f);
  for (int n = 0; n < N; ++n) {
    const int wi = n - left;
    win_h[n] = (wi >= 0 && wi < W) ? (float)(0.5 - 0.5 * std::cos(two_pi * wi / W)) : 0.f;
  }
  h->fb_host.resize((size_t)h->n_bins * c->n_mels);
  hfg_mel_filterbank(c, h->fb_host.data());
  h->fpw = N <= 1024 ? 2 : 1;
  int md = 0;  // 1: the DFT-GEMM path (A/B and fallback tests: hfg_debug_schedule_set)
  hfg_debug_schedule_get("MEL_DFT", &md);
  h->fft = (N & (N - 1)) == 0 && N >= 16 && md == 0 &&
           hfg::logmel_fft_lds_bytes(N, c->hop_length, h->fpw, c->n_mels) <= hfg::kMaxLdsBytes;
  if (!h->fft && !dft_fits) {
    delete h;
    return mfail(HFG_EINVAL, "n_fft / hop too large for the LDS frame tiles");
  }
  int rc = upload_tables(h, win_h.data(), h->fb_host.data());
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
  if (h->win) (void)hipFree(h->win);
  if (h->tw) (void)hipFree(h->tw);
  if (h->band) (void)hipFree(h->band);
  if (h->bw) (void)hipFree(h->bw);
  for (void* p : h->retired) (void)hipFree(p);
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
  int prev = -1;
  (void)hipGetDevice(&prev);
  if (prev != h->device && hipSetDevice(h->device) != hipSuccess)
    return mfail(HFG_ENODEV, "hipSetDevice(%d)", h->device);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int log_mode = h->cfg.log_base == 10 ? 1 : (h->cfg.log_base == 0 ? 0 : 2);
  // torch.log(torch.tensor(log_base)): a float32 log of the base
  const float ln_base = std::log(h->cfg.log_base_value);
  if (h->fft) {
    hipError_t e = hfg::launch_logmel_fft(wav, B, n_samples, h->cfg.n_fft, h->cfg.hop_length,
                                          n_frames, h->fpw, h->win, h->tw, h->band, h->bw,
                                          h->cfg.n_mels, h->cfg.log_eps, log_mode, ln_base, mel, s);
    if (prev >= 0 && prev != h->device) (void)hipSetDevice(prev);
    if (e != hipSuccess) return mfail(HFG_EIO, "mel launch: %s", hipGetErrorString(e));
    return HFG_OK;
  }
  float* power = reinterpret_cast<float*>(workspace);
  hipError_t e = hfg::launch_stft_power(wav, B, n_samples, h->cfg.n_fft, h->cfg.hop_length,
                                        h->n_bins, n_frames, h->tcos, h->tsin, h->bins_pad, power,
                                        s);
  if (e == hipSuccess)
    e = hfg::launch_mel_log(power, B, n_frames, h->n_bins, h->fb, h->cfg.n_mels, h->cfg.log_eps,
                            log_mode, ln_base, mel, s);
  if (prev >= 0 && prev != h->device) (void)hipSetDevice(prev);
  if (e != hipSuccess) return mfail(HFG_EIO, "mel launch: %s", hipGetErrorString(e));
  return HFG_OK;
}

}  // extern "C"

// ---- resampling (torchaudio.transforms.Resample, audio_processing.py:81-88) ----------
struct hfg_resample_handle {
  int orig, new_, g;          // reduced rates orig / g, new / g
  int width, klen;
  int device;
  float* kern = nullptr;      // [new][klen] on the device
  // hfg_resample_ragged: the same numbers tap-major, [klen][new], uploaded beside kern so the
  // call allocates nothing, and which of the two its kernel reads (schedule knob RESAMPLE_TABLE)
  float* kern_t = nullptr;
  bool tap_major = true;
};

namespace {
long long gcd_ll(long long a, long long b) {
  while (b) {
    const long long t = a % b;
    a = b;
    b = t;
  }
  return a;
}
}  // namespace

extern "C" {

// torchaudio.functional._get_sinc_resample_kernel(orig, new, gcd, lowpass_filter_width,
// rolloff, "sinc_interp_hann", dtype=None): float64 arithmetic (the phase offsets j/new
// are a float32 division of an integer tensor, as there), stored float32.
int hfg_resample_kernel(int32_t orig_freq, int32_t new_freq, int32_t lpw, float rolloff,
                        float* kernel, int32_t* width_out, int32_t* n_phases, int32_t* klen_out) {
  if (orig_freq <= 0 || new_freq <= 0 || lpw <= 0 || !(rolloff > 0.f && rolloff <= 1.f))
    return mfail(HFG_EINVAL, "resample: rates and lowpass_filter_width must be > 0, "
                 "0 < rolloff <= 1");
  const long long g = gcd_ll(orig_freq, new_freq);
  const long long orig = orig_freq / g, nw = new_freq / g;
  const double base = (double)std::min(orig, nw) * (double)rolloff;
  const int width = (int)std::ceil((double)lpw * (double)orig / base);
  const int klen = 2 * width + (int)orig;
  if (width_out) *width_out = width;
  if (n_phases) *n_phases = (int32_t)nw;
  if (klen_out) *klen_out = klen;
  if (!kernel) return HFG_OK;
  const double pi = 3.14159265358979323846;
  for (long long j = 0; j < nw; ++j) {
    const double off = (double)((float)(-j) / (float)nw);
    for (int k = 0; k < klen; ++k) {
      double t = (off + (double)(k - width) / (double)orig) * base;
      t = std::min((double)lpw, std::max(-(double)lpw, t));
      const double c = std::cos(t * pi / lpw / 2);
      const double window = c * c;
      t *= pi;
      const double v = (t == 0.0 ? 1.0 : std::sin(t) / t) * (window * (base / (double)orig));
      kernel[j * klen + k] = (float)v;
    }
  }
  return HFG_OK;
}

int hfg_resample_create(int32_t orig_freq, int32_t new_freq, int32_t lpw, float rolloff,
                        int device, hfg_resample_handle** out) {
  if (!out) return mfail(HFG_EINVAL, "out is NULL");
  *out = nullptr;
  int32_t width = 0, np = 0, klen = 0;
  int rc = hfg_resample_kernel(orig_freq, new_freq, lpw, rolloff, nullptr, &width, &np, &klen);
  if (rc) return rc;
  const long long g = gcd_ll(orig_freq, new_freq);
  // equal rates: torchaudio returns its input and hfg_resample_forward copies; the handle's
  // table is the identity (one phase, one tap of 1.0f, no pad), which hfg_resample_ragged runs
  // to convert, average and mask
  const bool same = orig_freq == new_freq;
  if (same) {
    width = 0;
    klen = 1;
  }
  if ((long long)np * klen > (1LL << 24))
    return mfail(HFG_EINVAL, "resample kernel [%d][%d] too large (rates %d -> %d)", np, klen,
                 orig_freq, new_freq);
  if ((size_t)((255 / np + 1) * (orig_freq / g) + klen) * sizeof(float) > 64 * 1024)
    return mfail(HFG_EINVAL, "resample ratio %d -> %d too large for the LDS input span",
                 orig_freq, new_freq);
  auto* h = new (std::nothrow) hfg_resample_handle();
  if (!h) return mfail(HFG_ENOMEM, "host alloc");
  h->orig = (int)(orig_freq / g);
  h->new_ = np;
  h->g = (int)g;
  h->width = width;
  h->klen = klen;
  h->device = device;
  if (device >= 0) {
    std::vector<float> k((size_t)np * klen), kt((size_t)np * klen);
    if (same)
      k[0] = 1.0f;
    else
      hfg_resample_kernel(orig_freq, new_freq, lpw, rolloff, k.data(), nullptr, nullptr, nullptr);
    for (int j = 0; j < np; ++j)
      for (int t = 0; t < klen; ++t) kt[(size_t)t * np + j] = k[(size_t)j * klen + t];
    int tm = 1;  // 0: hfg_resample_ragged reads the phase-major table (A/B: time_resample.py)
    hfg_debug_schedule_get("RESAMPLE_TABLE", &tm);
    h->tap_major = tm != 0;
    int prev = -1;
    (void)hipGetDevice(&prev);
    if (hipSetDevice(device) != hipSuccess) {
      delete h;
      return mfail(HFG_ENODEV, "hipSetDevice(%d)", device);
    }
    if (hipMalloc(&h->kern, k.size() * sizeof(float)) != hipSuccess ||
        hipMemcpy(h->kern, k.data(), k.size() * sizeof(float), hipMemcpyHostToDevice) !=
            hipSuccess ||
        hipMalloc(&h->kern_t, kt.size() * sizeof(float)) != hipSuccess ||
        hipMemcpy(h->kern_t, kt.data(), kt.size() * sizeof(float), hipMemcpyHostToDevice) !=
            hipSuccess) {
      hfg_resample_destroy(h);
      return mfail(HFG_ENOMEM, "resample kernel upload");
    }
    if (prev >= 0) (void)hipSetDevice(prev);
  }
  *out = h;
  return HFG_OK;
}

void hfg_resample_destroy(hfg_resample_handle* h) {
  if (!h) return;
  if (h->kern) (void)hipFree(h->kern);
  if (h->kern_t) (void)hipFree(h->kern_t);
  delete h;
}

int64_t hfg_resample_out_len(const hfg_resample_handle* h, int64_t n) {
  if (!h || n < 0) return -1;
  // torch.ceil(torch.as_tensor(new * length / orig)) on the reduced rates (a float64 quotient)
  return (int64_t)std::ceil((double)h->new_ * (double)n / (double)h->orig);
}

int hfg_resample_forward(hfg_resample_handle* h, const float* x, int64_t B, int64_t n, float* y,
                         void* stream) {
  if (!h || !x || !y) return mfail(HFG_EINVAL, "NULL argument");
  if (h->device < 0) return mfail(HFG_EINVAL, "host-only resample handle");
  if (B <= 0 || n <= 0) return mfail(HFG_EINVAL, "B and n_samples must be > 0");
  const int64_t n_out = hfg_resample_out_len(h, n);
  int prev = -1;
  (void)hipGetDevice(&prev);
  if (prev != h->device && hipSetDevice(h->device) != hipSuccess)
    return mfail(HFG_ENODEV, "hipSetDevice(%d)", h->device);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipError_t e;
  if (h->orig == h->new_)
    e = hipMemcpyAsync(y, x, sizeof(float) * (size_t)(B * n), hipMemcpyDeviceToDevice, s);
  else
    e = hfg::launch_resample(x, B, n, n_out, h->kern, h->new_, h->orig, h->klen, h->width, y, s);
  if (prev >= 0 && prev != h->device) (void)hipSetDevice(prev);
  if (e != hipSuccess) return mfail(HFG_EIO, "resample launch: %s", hipGetErrorString(e));
  return HFG_OK;
}

// include/hifigan_hip_resample.h: every argument is checked before any HIP call
int hfg_resample_ragged(hfg_resample_handle* h, const void* x, int dtype, int64_t B, int64_t C,
                        int64_t n_samples, const int32_t* lengths, float* y, int32_t* out_lengths,
                        void* stream) {
  const char* who = "hfg_resample_ragged";
  if (!h || !x || !y) return mfail(HFG_EINVAL, "%s: NULL argument", who);
  if (B < 1 || B > 65535) return mfail(HFG_EINVAL, "%s: B must be in [1, 65535]", who);
  if (C < 1 || C > HFG_RESAMPLE_MAX_CHANNELS)
    return mfail(HFG_EINVAL, "%s: C must be in [1, %d]", who, HFG_RESAMPLE_MAX_CHANNELS);
  if (n_samples < 1) return mfail(HFG_EINVAL, "%s: n_samples must be >= 1", who);
  if (dtype != HFG_PCM_S16 && dtype != HFG_PCM_F32)
    return mfail(HFG_EINVAL, "%s: dtype must be HFG_PCM_S16 (0) or HFG_PCM_F32 (1), got %d", who,
                 dtype);
  const int64_t n_out = n_samples > INT32_MAX ? -1 : hfg_resample_out_len(h, n_samples);
  if (n_out < 1 || n_out > INT32_MAX)
    return mfail(HFG_EINVAL, "%s: n_samples %lld and its output length must not exceed "
                 "INT32_MAX", who, (long long)n_samples);
  const size_t lds = hfg::resample_ragged_lds_bytes(C, h->new_, h->orig, h->klen);
  if (lds > hfg::kResampleRaggedMaxLds)
    return mfail(HFG_EINVAL, "%s: the input span of %lld channels (%zu bytes) does not fit the "
                 "%zu-byte LDS tile at this rate ratio", who, (long long)C, lds,
                 hfg::kResampleRaggedMaxLds);
  if (h->device < 0) return mfail(HFG_EINVAL, "%s: host-only resample handle", who);
  int prev = -1;
  (void)hipGetDevice(&prev);
  if (prev != h->device && hipSetDevice(h->device) != hipSuccess)
    return mfail(HFG_ENODEV, "hipSetDevice(%d)", h->device);
  const hipError_t e = hfg::launch_resample_ragged(
      x, dtype == HFG_PCM_S16, B, C, n_samples, lengths, n_out,
      h->tap_major ? h->kern_t : h->kern, h->tap_major, h->new_, h->orig, h->klen, h->width, y,
      out_lengths, reinterpret_cast<hipStream_t>(stream));
  if (prev >= 0 && prev != h->device) (void)hipSetDevice(prev);
  if (e != hipSuccess) return mfail(HFG_EIO, "%s launch: %s", who, hipGetErrorString(e));
  return HFG_OK;
}

}  // extern "C"

// ---- the public HiFi-GAN release's mel front end (include/hifigan_hip_relmel.h) ---------
// meldataset.mel_spectrogram: reflect pad (n_fft - hop) / 2, torch.stft(center=False),
// sqrt(re^2 + im^2 + 1e-9), librosa.filters.mel, ln(max(mel, 1e-5)); one launch of
// release_mel_fft (release_mel.hip), per-item lengths.
struct hfg_relmel_handle {
  hfg_relmel_config cfg;  // with fmax, spec_eps and clip_val resolved
  int device;
  int n_bins;
  int fpw;
  float* win = nullptr;   // [n_fft] fp32
  void* tw = nullptr;     // [n_fft] complex double
  int* band = nullptr;    // [num_mels] x (first bin, end bin, offset into bw)
  float* bw = nullptr;    // the bands' nonzero weights
  std::vector<void*> retired;  // replaced tables (a forward in flight may read them)
};

namespace {

// librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax) (htk=False, norm="slaney") in double:
// out[k][m], k < n_fft/2 + 1 (librosa's Slaney hz_to_mel / mel_to_hz are torchaudio's).
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
  for (int m = 0; m < n_mels; ++m) {
    const double enorm = 2.0 / (mel_f[m + 2] - mel_f[m]);
    for (int k = 0; k < n_bins; ++k) {
      const double lower = -(mel_f[m] - fftfreqs[k]) / (mel_f[m + 1] - mel_f[m]);
      const double upper = (mel_f[m + 2] - fftfreqs[k]) / (mel_f[m + 2] - mel_f[m + 1]);
      out[(size_t)k * n_mels + m] = (float)(std::fmax(0.0, std::fmin(lower, upper)) * enorm);
    }
  }
}

int relmel_upload(hfg_relmel_handle* h, const float* win, const float* fb) {
  const FftTables ft = fft_host_tables(h->cfg.n_fft, h->n_bins, h->cfg.num_mels, fb);
  if (h->device < 0) return HFG_OK;
  std::vector<Tbl> tbls;
  tbls.push_back({reinterpret_cast<void**>(&h->win), win, (size_t)h->cfg.n_fft * 4, nullptr});
  tbls.push_back({&h->tw, ft.tw.data(), ft.tw.size() * 8, nullptr});
  tbls.push_back({reinterpret_cast<void**>(&h->band), ft.band.data(), ft.band.size() * 4, nullptr});
  tbls.push_back({reinterpret_cast<void**>(&h->bw), ft.bw.data(), ft.bw.size() * 4, nullptr});
  return swap_tables(h->device, tbls, h->retired);
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
  h->n_bins = c.n_fft / 2 + 1;
  h->fpw = fpw;
  const int N = c.n_fft, W = c.win_size, left = (N - W) / 2;
  const double two_pi = 6.283185307179586476925286766559;
  std::vector<float> win_h(N, 0.f);
  for (int n = 0; n < N; ++n) {
    const int wi = n - left;
    win_h[n] = (wi >= 0 && wi < W) ? (float)(0.5 - 0.5 * std::cos(two_pi * wi / W)) : 0.f;
  }
  std::vector<float> fb_h((size_t)h->n_bins * c.num_mels);
  librosa_mel(&c, fb_h.data());
  int rc = relmel_upload(h, win_h.data(), fb_h.data());
  if (rc) {
    hfg_relmel_destroy(h);
    return rc;
  }
  *out = h;
  return HFG_OK;
}

void hfg_relmel_destroy(hfg_relmel_handle* h) {
  if (!h) return;
  if (h->win) (void)hipFree(h->win);
  if (h->tw) (void)hipFree(h->tw);
  if (h->band) (void)hipFree(h->band);
  if (h->bw) (void)hipFree(h->bw);
  for (void* p : h->retired) (void)hipFree(p);
  delete h;
}

int hfg_relmel_set_tables(hfg_relmel_handle* h, const float* window, const float* fb) {
  if (!h || !window || !fb) return mfail(HFG_EINVAL, "NULL argument");
  return relmel_upload(h, window, fb);
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
  int prev = -1;
  (void)hipGetDevice(&prev);
  if (prev != h->device && hipSetDevice(h->device) != hipSuccess)
    return mfail(HFG_ENODEV, "hipSetDevice(%d)", h->device);
  hipError_t e = hfg::launch_release_mel_fft(
      wav, B, n_samples, lengths, h->cfg.n_fft, h->cfg.hop_size, h->fpw, h->win, h->tw, h->band,
      h->bw, h->cfg.num_mels, h->cfg.spec_eps, h->cfg.clip_val, mel, frame_lengths,
      reinterpret_cast<hipStream_t>(stream));
  if (prev >= 0 && prev != h->device) (void)hipSetDevice(prev);
  if (e != hipSuccess) return mfail(HFG_EIO, "release mel launch: %s", hipGetErrorString(e));
  return HFG_OK;
}

}  // extern "C"

// ---- the release's PCM boundary (include/hifigan_hip_pcm.h) -----------------------------
// Stateless: arguments are checked before any HIP call, then one launch of pcm.hip on the
// caller's stream (hfg_pcm_peak: one memset in front of it).
namespace {

int pcm_check(const char* who, int64_t B, int64_t n_samples) {
  if (B < 1 || B > 65535) return mfail(HFG_EINVAL, "%s: B must be in [1, 65535]", who);
  if (n_samples < 1) return mfail(HFG_EINVAL, "%s: n_samples must be >= 1", who);
  return HFG_OK;
}
int pcm_dtype(const char* who, int dtype) {
  if (dtype != HFG_PCM_S16 && dtype != HFG_PCM_F32)
    return mfail(HFG_EINVAL, "%s: dtype must be HFG_PCM_S16 (0) or HFG_PCM_F32 (1), got %d", who,
                 dtype);
  return HFG_OK;
}
int pcm_done(const char* who, hipError_t e) {
  return e == hipSuccess ? HFG_OK : mfail(HFG_EIO, "%s launch: %s", who, hipGetErrorString(e));
}

}  // namespace

extern "C" {

int hfg_pcm_peak(const void* wav, int dtype, int64_t B, int64_t n_samples,
                 const int32_t* lengths, float* peak, void* stream) {
  if (!wav || !peak) return mfail(HFG_EINVAL, "hfg_pcm_peak: NULL argument");
  if (int rc = pcm_check("hfg_pcm_peak", B, n_samples)) return rc;
  if (int rc = pcm_dtype("hfg_pcm_peak", dtype)) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(peak, 0, sizeof(float) * (size_t)B, s);
  if (e == hipSuccess)
    e = hfg::launch_pcm_peak(wav, dtype == HFG_PCM_S16, B, n_samples, lengths, peak, s);
  return pcm_done("hfg_pcm_peak", e);
}

int hfg_pcm_to_float(const void* wav, int dtype, int64_t B, int64_t n_samples,
                     const int32_t* lengths, const float* peak, double gain, float* out,
                     void* stream) {
  if (!wav || !out) return mfail(HFG_EINVAL, "hfg_pcm_to_float: NULL argument");
  if (int rc = pcm_check("hfg_pcm_to_float", B, n_samples)) return rc;
  if (int rc = pcm_dtype("hfg_pcm_to_float", dtype)) return rc;
  if (!std::isfinite(gain)) return mfail(HFG_EINVAL, "hfg_pcm_to_float: gain must be finite");
  return pcm_done("hfg_pcm_to_float",
                  hfg::launch_pcm_to_float(wav, dtype == HFG_PCM_S16, B, n_samples, lengths, peak,
                                           gain, out, reinterpret_cast<hipStream_t>(stream)));
}

int hfg_pcm_offsets(const int32_t* lengths, int64_t B, int64_t n_samples, int64_t* offsets,
                    void* stream) {
  if (!offsets) return mfail(HFG_EINVAL, "hfg_pcm_offsets: NULL argument");
  if (int rc = pcm_check("hfg_pcm_offsets", B, n_samples)) return rc;
  return pcm_done("hfg_pcm_offsets",
                  hfg::launch_pcm_offsets(lengths, B, n_samples, offsets,
                                          reinterpret_cast<hipStream_t>(stream)));
}

int hfg_pcm_from_float(const float* wav, int64_t B, int64_t n_samples, const int32_t* lengths,
                       int rounding, const int64_t* offsets, int16_t* out, void* stream) {
  if (!wav || !out) return mfail(HFG_EINVAL, "hfg_pcm_from_float: NULL argument");
  if (int rc = pcm_check("hfg_pcm_from_float", B, n_samples)) return rc;
  if (rounding != HFG_PCM_TRUNC && rounding != HFG_PCM_NEAREST)
    return mfail(HFG_EINVAL, "hfg_pcm_from_float: rounding must be HFG_PCM_TRUNC (0) or "
                 "HFG_PCM_NEAREST (1), got %d", rounding);
  return pcm_done("hfg_pcm_from_float",
                  hfg::launch_pcm_from_float(wav, B, n_samples, lengths,
                                             rounding == HFG_PCM_NEAREST, offsets, out,
                                             reinterpret_cast<hipStream_t>(stream)));
}

}  // extern "C"

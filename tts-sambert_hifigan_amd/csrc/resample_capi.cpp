// resample_capi.cpp — C ABI of the resampler (torchaudio.transforms.Resample,
// audio_processing.py:81-88): hfg_resample_* of include/hifigan_hip.h and the ragged
// multi-channel call of include/hifigan_hip_resample.h.  Kernels: resample.hip.
#include <algorithm>
#include <cmath>

#include "../../include/hifigan_hip_inspect.h"
#include "../../include/hifigan_hip_pcm.h"
#include "../../include/hifigan_hip_resample.h"
#include "frontend_host.h"

using namespace hfg_host;

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
  if (hfg::resample_lds_bytes(1, np, (int)(orig_freq / g), klen) > hfg::kResampleMaxLds)
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
    DeviceGuard dg(device);
    if (!dg.ok) {
      delete h;
      return mfail(HFG_ENODEV, "hipSetDevice(%d)", device);
    }
    auto up = [](float** d, const std::vector<float>& v) {
      return hipMalloc(d, v.size() * sizeof(float)) == hipSuccess &&
             hipMemcpy(*d, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice) == hipSuccess;
    };
    if (!up(&h->kern, k) || !up(&h->kern_t, kt)) {
      hfg_resample_destroy(h);
      return mfail(HFG_ENOMEM, "resample kernel upload");
    }
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
  DeviceGuard g(h->device);
  if (!g.ok) return mfail(HFG_ENODEV, "hipSetDevice(%d)", h->device);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipError_t e;
  if (h->orig == h->new_)
    e = hipMemcpyAsync(y, x, sizeof(float) * (size_t)(B * n), hipMemcpyDeviceToDevice, s);
  else
    e = hfg::launch_resample(x, B, n, n_out, h->kern, h->new_, h->orig, h->klen, h->width, y, s);
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
  const size_t lds = hfg::resample_lds_bytes(C, h->new_, h->orig, h->klen);
  if (lds > hfg::kResampleMaxLds)
    return mfail(HFG_EINVAL, "%s: the input span of %lld channels (%zu bytes) does not fit the "
                 "%zu-byte LDS tile at this rate ratio", who, (long long)C, lds,
                 hfg::kResampleMaxLds);
  if (h->device < 0) return mfail(HFG_EINVAL, "%s: host-only resample handle", who);
  DeviceGuard g(h->device);
  if (!g.ok) return mfail(HFG_ENODEV, "hipSetDevice(%d)", h->device);
  const hipError_t e = hfg::launch_resample_ragged(
      x, dtype == HFG_PCM_S16, B, C, n_samples, lengths, n_out,
      h->tap_major ? h->kern_t : h->kern, h->tap_major, h->new_, h->orig, h->klen, h->width, y,
      out_lengths, reinterpret_cast<hipStream_t>(stream));
  if (e != hipSuccess) return mfail(HFG_EIO, "%s launch: %s", who, hipGetErrorString(e));
  return HFG_OK;
}

}  // extern "C"

// pcm_capi.cpp — C ABI of the release's PCM boundary (include/hifigan_hip_pcm.h).
// Stateless: arguments are checked before any HIP call, then one launch of pcm.hip on the
// caller's stream (hfg_pcm_peak: one memset in front of it).
#include <cmath>

#include "../../include/hifigan_hip_pcm.h"
#include "frontend_host.h"

using namespace hfg_host;

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

/*
 * hifigan_hip_pcm.h — the PCM boundary of the public HiFi-GAN release on the device: what
 * its data loader does in front of mel_spectrogram (meldataset.py: 16-bit PCM divided by
 * MAX_WAV_VALUE, librosa.util.normalize(audio) * 0.95) and what inference.py does behind
 * the Generator (audio * MAX_WAV_VALUE, cast to int16).  Included by hifigan_hip.h; the entry
 * points live in libhifigan_hip.so.
 *
 * Stateless functions, no handle.  Every call is asynchronous on the caller's stream, on the
 * current device: no workspace, no allocation, no synchronisation (capturable into a
 * hipGraph); apart from the one memset of the peak entry each issues only its kernel.
 * Arguments are checked before any HIP call; errors are read with hfg_mel_last_error().
 * HFG_EINVAL: a NULL data pointer, B outside [1, 65535], n_samples < 1, an unknown dtype or
 * rounding code, a non-finite gain.
 *
 * Rows are dense: wav[B][n_samples].  `lengths` (device int32 [B], or NULL: every item has
 * n_samples) gives each item's valid samples; the kernels clamp len_b into [0, n_samples] and
 * never read a sample at or past len_b.
 *
 *   peak        peak[b] = max |x| over [0, len_b) as float32.  int16: the magnitude is taken
 *               in int32 (|-32768| = 32768) and divided by 32768, exact.  A NaN sample inside
 *               an item's length makes that item's peak NaN (numpy.max), no other item's;
 *               len_b = 0 gives 0.  peak[B] is zeroed first by one memset on the stream.
 *   to_float    out[b][i] = 0 for i >= len_b, else
 *                 peak NULL:  (float) s / 32768 (int16, exact; read_wav's value) or x (float32)
 *                 peak given: (float)(((double) v / d) * gain), v = (double) s / 32768.0 or
 *                             (double) x, d = (double) peak[b], or 1.0 where peak[b] is below
 *                             the smallest normal number of the input's float type (float64
 *                             for int16, so only peak 0; FLT_MIN for float32):
 *                             librosa.util.normalize's rule.
 *               One float64 division, one float64 product, one rounding: bitwise what numpy
 *               gives for torch.FloatTensor(normalize(audio / 32768.0) * gain).
 *   offsets     offsets[0] = 0, offsets[b + 1] = len_0 + ... + len_b (clamped lengths).
 *   from_float  q = sat16(round(x * 32768.0f)) for i < len_b.  HFG_PCM_TRUNC rounds toward
 *               zero (the release's astype('int16')), HFG_PCM_NEAREST to nearest even; sat16
 *               clamps to [-32768, 32767]; NaN gives 0.  offsets NULL: out[B][n_samples],
 *               0 for i >= len_b.  offsets given (as hfg_pcm_offsets wrote them for the same
 *               lengths): only out[offsets[b] + i], i < len_b, is written.
 *
 * Saturation differs from the release on purpose: there +1.0, which a tanh output reaches,
 * becomes 32768 and wraps to -32768; here it is 32767.
 */
#ifndef HIFIGAN_HIP_PCM_H
#define HIFIGAN_HIP_PCM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { HFG_PCM_S16 = 0, HFG_PCM_F32 = 1 };       /* dtype of wav */
enum { HFG_PCM_TRUNC = 0, HFG_PCM_NEAREST = 1 }; /* rounding */

int hfg_pcm_peak(const void* wav, int dtype, int64_t B, int64_t n_samples,
                 const int32_t* lengths, float* peak, void* stream);
int hfg_pcm_to_float(const void* wav, int dtype, int64_t B, int64_t n_samples,
                     const int32_t* lengths, const float* peak /* NULL: no normalisation */,
                     double gain, float* out, void* stream);
int hfg_pcm_offsets(const int32_t* lengths, int64_t B, int64_t n_samples,
                    int64_t* offsets /* [B+1] */, void* stream);
int hfg_pcm_from_float(const float* wav, int64_t B, int64_t n_samples, const int32_t* lengths,
                       int rounding, const int64_t* offsets /* NULL: padded [B][n_samples] */,
                       int16_t* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIFIGAN_HIP_PCM_H */

/*
 * hifigan_hip_resample.h — ragged, multi-channel resampling to mono on the device: what the
 * reference's front end does before it frames (data/audio_processing.py:81-94: resample every
 * channel to the model rate, then the mean over channels), for a padded batch whose items
 * have their own lengths, in one launch.  The first step of the release chain
 * (hfg_resample_ragged -> hfg_pcm_to_float -> hfg_relmel_forward -> hfg_forward_ex ->
 * hfg_pcm_from_float), which it feeds lengths that never visit the host.  Included by
 * hifigan_hip.h; the entry point lives in libhifigan_hip.so and works on the resample handle
 * declared there.
 *
 * Asynchronous on the caller's stream: no workspace, no allocation, no synchronisation, one
 * kernel (capturable into a hipGraph).  Arguments are checked before any HIP call; errors are
 * read with hfg_mel_last_error().  HFG_EINVAL, with nothing written: a NULL h, x or y, B
 * outside [1, 65535], C outside [1, HFG_RESAMPLE_MAX_CHANNELS], n_samples < 1, an unknown
 * dtype, n_samples or its output length above INT32_MAX, a channel count whose staged input
 * does not fit the kernel's 64 KiB LDS tile at the handle's ratio (C = 8 fits at every ratio
 * whose 256-output span is at most 2048 samples, e.g. 96000 -> 22050), a host-only handle
 * (checked last).
 *
 *   x            [B][C][n_samples], dense, planar channels, int16 (HFG_PCM_S16) or float32
 *                (HFG_PCM_F32: hifigan_hip_pcm.h).
 *   lengths      device int32 [B], or NULL: every item has n_samples.  len_b = lengths[b]
 *                clamped into [0, n_samples]; no sample at or past len_b is read.
 *   y            [B][n_out], n_out = hfg_resample_out_len(h, n_samples).  With the handle's
 *                reduced rates orig, new and its table kernel[new][klen], width (all as
 *                hfg_resample_kernel gives them) and out_len_b = ceil(new * len_b / orig):
 *                  m < out_len_b:  chain_c(m) = the sequential fp32 fma chain, from 0.f, over
 *                    k = 0 .. klen - 1 of xz_c[(m / new) * orig - width + k] * kernel[m % new][k],
 *                    xz_c = channel c of item b, zero outside [0, len_b), an int16 sample
 *                    entering as (float) s / 32768 (exact): hfg_resample_forward's sum on the
 *                    item cropped to its own length, bit for bit.
 *                    C = 1: y[b][m] = chain_0(m).
 *                    C > 1: y[b][m] = (((chain_0 + chain_1) + ...) + chain_{C-1}) / (float) C,
 *                    fp32 sums in channel order and one IEEE division.
 *                  out_len_b <= m < n_out:  y[b][m] = 0.
 *   out_lengths  device int32 [B], or NULL: receives out_len_b.
 *
 * Equal rates: hfg_resample_create accepts them (hfg_resample_forward then copies, as
 * torchaudio returns its input); the handle's table is the identity, one phase with the single
 * tap 1.0f and no pad.  hfg_resample_ragged runs it like any other table, so it still
 * converts, averages the channels and masks: for C = 1, y = x inside each length, except that
 * -0.0 comes out as +0.0 (the chain is 0.f + x * 1.0f).
 */
#ifndef HIFIGAN_HIP_RESAMPLE_H
#define HIFIGAN_HIP_RESAMPLE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { HFG_RESAMPLE_MAX_CHANNELS = 8 };

int hfg_resample_ragged(hfg_resample_handle* h, const void* x,
                        int dtype /* HFG_PCM_S16 | HFG_PCM_F32 */, int64_t B, int64_t C,
                        int64_t n_samples, const int32_t* lengths,
                        float* y /* [B][hfg_resample_out_len(h, n_samples)] */,
                        int32_t* out_lengths /* NULL allowed */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIFIGAN_HIP_RESAMPLE_H */

/*
 * hifigan_hip_specdist.h — forward-only spectral distances on the device: how far the mel of
 * a waveform is from a mel tensor the caller already holds (the mel fed to the Generator, an
 * acoustic model's prediction, the front end's own output in copy-synthesis), and the
 * multi-resolution log-STFT distance of two waveforms.  Included by hifigan_hip.h; the entry
 * points live in libhifigan_hip.so.  These are the two discriminator-free terms of the
 * reference's VocoderLoss (models/losses.py: mel_reconstruction_loss, compute_stft_loss) as
 * metrics: no gradients.
 *
 * Every forward is two launches on the caller's stream (the distance kernel, then a small
 * reduction), allocates nothing, does not synchronise, and is capturable into a hipGraph.
 * Errors are read with hfg_mel_last_error().
 *
 * Results, per item b of the batch:
 *   sums[2 b]     sum |d|  over the item's compared entries (float64)
 *   sums[2 b + 1] sum d^2                                   (float64)
 *   frames[b]     the item's compared frames (int32); entries = rows * frames[b], rows =
 *                 num_mels / n_mels, or n_fft / 2 + 1 for the STFT distance
 * The sums are deterministic: no floating-point atomics, a fixed summation order, and blocks
 * past an item's frames add an exact 0.0, so item b's sums are bitwise those of a call on item
 * b alone and bitwise the same on every call.  `workspace` ([B][blocks] pairs of doubles)
 * needs no initialisation.
 *
 * Ragged batches: `lengths` (device int32 [B], or NULL: every item has n_samples) is clamped
 * into [0, n_samples] by the kernel; item b is framed as if it were alone with len_b samples,
 * and samples at or past len_b are never read.
 *
 * Mel distance, d = v - target[b][m][f] with v the float32 value hfg_relmel_forward /
 * hfg_mel_forward would have stored (no mel is written).  target: [B][rows][target_cols]
 * float32 on the device.  Item b's compared frames are F_b = min(frames(len_b), target_cols),
 * frames(len) = len / hop for the release framing (0 unless len > (n_fft - hop) / 2 and
 * len >= hop) and len / hop + 1 for hfg_mel (0 unless len > n_fft / 2); target columns at or
 * past F_b are never read.  An hfg_mel handle on the DFT-GEMM path (n_fft not a power of two)
 * is refused with HFG_EINVAL.
 *
 * STFT distance, d = (float) ln(|STFT a| + eps) - (float) ln(|STFT b| + eps) over bins
 * 0..n_fft/2 of every frame: torch.stft(center=True, reflect pad, the periodic Hann window of
 * win_length centred in n_fft), float64 FFT.  Item b has len_b / hop + 1 frames when
 * len_b > n_fft / 2, else 0.  One handle per resolution.
 *
 * HFG_EINVAL: a NULL pointer (lengths excepted), B outside [1, 65535], an n_samples with no
 * frame, a host-only handle, workspace_bytes below *_workspace_bytes(h, B, n_samples),
 * target_cols < 1.
 */
#ifndef HIFIGAN_HIP_SPECDIST_H
#define HIFIGAN_HIP_SPECDIST_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

size_t hfg_relmel_distance_workspace_bytes(const hfg_relmel_handle* h, int64_t B,
                                           int64_t n_samples);
int hfg_relmel_distance(hfg_relmel_handle* h, const float* wav, int64_t B, int64_t n_samples,
                        const int32_t* lengths, const float* target, int64_t target_cols,
                        void* workspace, size_t workspace_bytes, double* sums, int32_t* frames,
                        void* stream);

size_t hfg_mel_distance_workspace_bytes(const hfg_mel_handle* h, int64_t B, int64_t n_samples);
int hfg_mel_distance(hfg_mel_handle* h, const float* wav, int64_t B, int64_t n_samples,
                     const int32_t* lengths, const float* target, int64_t target_cols,
                     void* workspace, size_t workspace_bytes, double* sums, int32_t* frames,
                     void* stream);

typedef struct hfg_stftdist_handle hfg_stftdist_handle;
typedef struct hfg_stftdist_config {
    int32_t n_fft;        /* a power of two >= 16 whose frame tile fits the LDS (<= 2048) */
    int32_t hop_length;   /* >= 1                                                        */
    int32_t win_length;   /* 1..n_fft                                                    */
    float eps;            /* 0: 1e-5 (the reference's)                                   */
} hfg_stftdist_config;

/* device -1: a host-only handle (configuration checks, frame counts, workspace sizes).  The
 * handle's default window is the periodic Hann window of win_length centred in n_fft,
 * evaluated in double and rounded to fp32. */
int hfg_stftdist_create(const hfg_stftdist_config* cfg, int device, hfg_stftdist_handle** out);
void hfg_stftdist_destroy(hfg_stftdist_handle* h);
/* Replace the window [n_fft] (host pointer, fp32), e.g. by torch.hann_window's float32 values:
 * next to eps = 1e-5 a one-ulp window difference moves the log magnitude of quiet bins by more
 * than the float32 rounding of the result. */
int hfg_stftdist_set_window(hfg_stftdist_handle* h, const float* window);
/* n_samples / hop_length + 1; -1 if n_samples <= n_fft / 2 */
int64_t hfg_stftdist_frames(const hfg_stftdist_handle* h, int64_t n_samples);
size_t hfg_stftdist_workspace_bytes(const hfg_stftdist_handle* h, int64_t B, int64_t n_samples);
/* a, b: [B][n_samples] float32 on the device, sharing `lengths` */
int hfg_stftdist_forward(hfg_stftdist_handle* h, const float* a, const float* b, int64_t B,
                         int64_t n_samples, const int32_t* lengths, void* workspace,
                         size_t workspace_bytes, double* sums, int32_t* frames, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIFIGAN_HIP_SPECDIST_H */
